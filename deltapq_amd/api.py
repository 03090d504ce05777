"""Python face of the C-ABI (include/deltapq_amd.h) for tests, bench.py and the
multi-GPU driver.  Everything here is plumbing: numpy/torch buffers in, the HIP
library does the work.  Names of the two convenience functions at the bottom
mirror the reference's entry points (deltapq_create_approx_tree.h:2805, 3731).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import DpqError, Info, OpenOpts, Profile, check  # noqa: F401


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def device_count():
    return _lib.load().dpq_device_count()


def read_codewords(path):
    """PQ::ReadCodewords (pq.cpp:288-312) -> float32 [M][K][Ds]."""
    lib = _lib.load()
    M, K, Ds = _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
    check(lib.dpq_read_codewords(path.encode(), M, K, Ds, None), "dpq_read_codewords")
    out = np.empty((M.value, K.value, Ds.value), dtype=np.float32)
    check(lib.dpq_read_codewords(path.encode(), M, K, Ds, _np_ptr(out)), "dpq_read_codewords")
    return out


def read_vecs(path, ext="fvecs", top_n=-1):
    """ReadTopN (utils.cpp:96-110) over .fvecs/.bvecs -> float32 [n][D]."""
    lib = _lib.load()
    n, D = _lib.c_i64(), _lib.c_i32()
    check(lib.dpq_read_vecs(path.encode(), int(ext == "bvecs"), n, D, None, 0), "dpq_read_vecs")
    keep = n.value if top_n < 0 else min(n.value, top_n)
    out = np.empty((keep, D.value), dtype=np.float32)
    check(lib.dpq_read_vecs(path.encode(), int(ext == "bvecs"), n, D, _np_ptr(out), keep), "dpq_read_vecs")
    return out


def read_dtc_file(path):
    """(n_codes, payload u8[n_bytes]) of a reference DTC index file (h:1839-1842)."""
    lib = _lib.load()
    n_codes, n_bytes = _lib.c_i64(), _lib.c_i64()
    check(lib.dpq_read_dtc_header(path.encode(), n_codes, n_bytes), "dpq_read_dtc_header")
    payload = np.fromfile(path, dtype=np.uint8, offset=16, count=n_bytes.value)
    return n_codes.value, payload


def dtc_validate(payload, n_codes, M=8):
    lib = _lib.load()
    pl = np.ascontiguousarray(payload, dtype=np.uint8)
    st = _lib.DtcStats()
    check(lib.dpq_dtc_validate(_np_ptr(pl), pl.size, n_codes, M, st), "dpq_dtc_validate")
    return dict(n_codes=st.n_codes, n_bytes=st.n_bytes, n_diffs=st.n_diffs, max_depth=st.max_depth,
                depth_hist=list(st.depth_hist))


def dtc_encode(root, depths, masks, deltas, M=8):
    """qnodes_to_compressed_codes_opt (h:1765-1826) through the C-ABI."""
    lib = _lib.load()
    root = np.ascontiguousarray(root, dtype=np.uint8)
    depths = np.ascontiguousarray(depths, dtype=np.uint8)
    masks = np.ascontiguousarray(masks, dtype=np.uint16)
    deltas = np.ascontiguousarray(deltas, dtype=np.uint8)
    nb = _lib.c_i64()
    check(lib.dpq_dtc_encode(_np_ptr(root), _np_ptr(depths), _np_ptr(masks), _np_ptr(deltas), len(depths), M, None,
                             nb), "dpq_dtc_encode")
    out = np.empty(nb.value, dtype=np.uint8)
    check(lib.dpq_dtc_encode(_np_ptr(root), _np_ptr(depths), _np_ptr(masks), _np_ptr(deltas), len(depths), M,
                             _np_ptr(out), nb), "dpq_dtc_encode")
    return out


def dtc_decode(payload, n_codes, M=8, first=0, count=None):
    """The inverse of dtc_encode (dpq_dtc_decode): codes [first, first + count) of a DTC payload in DFS order,
    uint8 [count][M].  count=None: everything from `first` on.  Positions, not reported ids."""
    lib = _lib.load()
    pl = np.ascontiguousarray(payload, dtype=np.uint8)
    if count is None:
        count = n_codes - first
    out = np.empty((max(int(count), 0), M), dtype=np.uint8)
    check(lib.dpq_dtc_decode(_np_ptr(pl), pl.size, n_codes, M, first, count, _np_ptr(out)), "dpq_dtc_decode")
    return out


class HostSoA:
    """The transcoded structure-of-arrays image, built on the host (no GPU)."""

    def __init__(self, payload, n_codes, M=8, shard_rank=0, shard_count=1, chunks_per_segment=0, num_codes=0,
                 multi_index_stride=0):
        lib = _lib.load()
        pl = np.ascontiguousarray(payload, dtype=np.uint8)
        opts = OpenOpts(0, shard_rank, shard_count, chunks_per_segment, 0, num_codes, multi_index_stride)
        h = ctypes.c_void_p()
        check(lib.dpq_soa_build(_np_ptr(pl), pl.size, n_codes, M, opts, h), "dpq_soa_build")
        self._h = h
        info = Info()
        check(lib.dpq_soa_info(h, info), "dpq_soa_info")
        self.info = info.as_dict()
        names = ["nib", "mask", "delta", "seg_delta_off", "seg_ckpt", "mi_cell_start", "mi_code", "mi_id", "par", "carry",
                 "st_ckpt", "st_mask", "st_poff", "st_pbase", "st_delta", "st_depth"]
        views = {"seg_delta_off": np.uint64, "st_ckpt": np.uint64, "st_mask": np.uint32, "st_poff": np.uint16, "st_pbase": np.uint32,
                 "st_depth": np.uint16}
        for which, name in enumerate(names):
            ptr, nb = ctypes.c_void_p(), _lib.c_i64()
            check(lib.dpq_soa_array(h, which, ptr, nb), "dpq_soa_array")
            buf = (ctypes.c_ubyte * nb.value).from_address(ptr.value) if nb.value else b""
            arr = np.frombuffer(buf, dtype=np.uint8).copy()
            if name in views:
                arr = arr.view(views[name])
            if name.startswith("mi_"):
                arr = arr.view(np.uint32)
            setattr(self, name, arr)
        lib.dpq_soa_free(h)
        self._h = None


class DeltaTree:
    """DeltaTree built from raw PQ codes on the host (`deltapq -task approx_tree`, method 1;
    create_approx_tree, deltapq_create_approx_tree.h:970-1065)."""

    _ARRAYS = [("vec_id", np.uint32), ("parent_pos", np.uint32), ("depth", np.uint8), ("mask", np.uint16),
               ("deltas", np.uint8), ("root", np.uint8), ("edges", np.uint32)]

    def __init__(self, codes, K=256, max_height_folds=1, codebook=None, device=None):
        """device=None: everything on the host; device=i: the edge search runs on GPU i
        (dpq_tree_build_gpu) and yields the same tree."""
        lib = _lib.load()
        self._lib = lib
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        assert c.ndim == 2
        n, M = c.shape
        cb = None if codebook is None else np.ascontiguousarray(codebook, dtype=np.float32)
        h = ctypes.c_void_p()
        cbp, ds = (None, 0) if cb is None else (_np_ptr(cb), cb.shape[2])
        if device is None:
            check(lib.dpq_tree_build(_np_ptr(c), n, M, K, max_height_folds, cbp, ds, h), "dpq_tree_build")
        else:
            check(lib.dpq_tree_build_gpu(_np_ptr(c), n, M, K, max_height_folds, cbp, ds, device, h),
                  "dpq_tree_build_gpu")
        self._h = h
        self.M, self.K, self.n = M, K, n
        st = _lib.DtcStats()
        check(lib.dpq_tree_stats(h, st), "dpq_tree_stats")
        self.stats = dict(n_codes=st.n_codes, n_bytes=st.n_bytes, n_diffs=st.n_diffs, max_depth=st.max_depth,
                          depth_hist=list(st.depth_hist))
        for which, (name, dt) in enumerate(self._ARRAYS):
            ptr, nb = ctypes.c_void_p(), _lib.c_i64()
            check(lib.dpq_tree_array(h, which, ptr, nb), "dpq_tree_array")
            buf = (ctypes.c_ubyte * nb.value).from_address(ptr.value) if nb.value else b""
            setattr(self, name, np.frombuffer(buf, dtype=np.uint8).copy().view(dt))
        self.edges = self.edges.reshape(-1, 2)

    def payload(self):
        nb = _lib.c_i64()
        check(self._lib.dpq_tree_encode(self._h, None, nb), "dpq_tree_encode")
        out = np.empty(nb.value, dtype=np.uint8)
        check(self._lib.dpq_tree_encode(self._h, _np_ptr(out), nb), "dpq_tree_encode")
        return out

    def write_files(self, dataset_dir):
        check(self._lib.dpq_tree_write_files(self._h, dataset_dir.encode()), "dpq_tree_write_files")

    def close(self):
        if self._h is not None:
            self._lib.dpq_tree_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_pq(vectors, codebook, device=0):
    """PQTree::EncodePlain (pq_tree.cpp:215-237) on the GPU: uint8 codes [n][M]."""
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    cb = np.ascontiguousarray(codebook, dtype=np.float32)
    M, K, Ds = cb.shape
    out = np.empty((v.shape[0], M), dtype=np.uint8)
    check(lib.dpq_encode_pq(_np_ptr(v), v.shape[0], v.shape[1], _np_ptr(cb), M, K, Ds, device, _np_ptr(out)),
          "dpq_encode_pq")
    return out


_TRAIN_STARTS = {"rows": 0, "kmeans++": 1}


def train_codebook(vectors, M=8, K=256, max_iters=25, seed=0, init=None, device=0, start="rows", restarts=1):
    """Codebook learning on the GPU (dpq_train_codebook; replaces PQ::Learn, pq.cpp:112-157, with this build's own
    exact semantics -- no reference semantics (cv::kmeans)).  init: a start [M][K][Ds] instead of the seeded one.
    start: "rows" (K random rows, the same for every sub-space) or "kmeans++" (per sub-space, on the GPU).
    restarts: that many independent runs with seed, seed + 1, ...; every sub-space keeps the run with the lowest
    potential.  Returns (codebook float32 [M][K][Ds], stats dict)."""
    if start not in _TRAIN_STARTS:
        raise ValueError('start must be "rows" or "kmeans++"')
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert v.ndim == 2
    n, D = v.shape
    Ds = -(-D // M) if M >= 1 else 1
    opts = _lib.TrainOpts(device=device, max_iters=max_iters, seed=seed, use_initial=int(init is not None),
                          init=_TRAIN_STARTS[start], restarts=restarts)
    if init is None:
        cb = np.zeros((max(M, 1), max(K, 1), Ds), dtype=np.float32)
    else:
        cb = np.array(init, dtype=np.float32, order="C")
        assert cb.shape == (M, K, Ds), "init must be [M][K][ceil(D / M)]"
    st = _lib.TrainStats()
    check(lib.dpq_train_codebook(_np_ptr(v), n, D, M, K, opts, _np_ptr(cb), st), "dpq_train_codebook")
    stats = {k: getattr(st, k) for k, _ in st._fields_ if k != "distortion"}
    stats["distortion"] = [st.distortion[i] for i in range(st.iters_run)]
    return cb, stats


def kmeanspp_seed(vectors, M=8, K=256, seed=0, device=0):
    """The k-means++ start alone (dpq_kmeanspp_seed): (codebook float32 [M][K][Ds], potential float64 [M])."""
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert v.ndim == 2
    n, D = v.shape
    cb = np.zeros((max(M, 1), max(K, 1), -(-D // M) if M >= 1 else 1), dtype=np.float32)
    pot = np.zeros(max(M, 1), dtype=np.float64)
    check(lib.dpq_kmeanspp_seed(_np_ptr(v), n, D, M, K, seed, device, _np_ptr(cb), _np_ptr(pot)), "dpq_kmeanspp_seed")
    return cb, pot


def train_potential(vectors, codebook, device=0):
    """The leaf-ordered potential of a codebook per sub-space (dpq_train_potential): float64 [M], the sum of the
    winning distances in the order the header states, so two codebooks compare reproducibly."""
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    cb = np.ascontiguousarray(codebook, dtype=np.float32)
    assert v.ndim == 2 and cb.ndim == 3
    M, K, Ds = cb.shape
    pot = np.zeros(M, dtype=np.float64)
    check(lib.dpq_train_potential(_np_ptr(v), v.shape[0], v.shape[1], _np_ptr(cb), M, K, Ds, device, _np_ptr(pot)),
          "dpq_train_potential")
    return pot


def write_codewords(path, codebook):
    """PQ::WriteCodewords' format (pq.cpp:267-286) with nine significant digits: read_codewords gives the same bits."""
    cb = np.ascontiguousarray(codebook, dtype=np.float32)
    M, K, Ds = cb.shape
    check(_lib.load().dpq_write_codewords(path.encode(), _np_ptr(cb), M, K, Ds), "dpq_write_codewords")


def rotate(vectors, rotation, device=0):
    """out = vectors . rotation on the GPU (dpq_rotate): fp64 accumulation over d ascending, rounded once to float32.
    Host arrays; returns float32 [n][D]."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if v.ndim == 1:
        v = v[None, :]
    r = np.ascontiguousarray(rotation, dtype=np.float32)
    assert v.ndim == 2 and r.shape == (v.shape[1], v.shape[1]), "rotation must be [D][D]"
    out = np.empty_like(v)
    check(_lib.load().dpq_rotate(_np_ptr(v), v.shape[0], v.shape[1], _np_ptr(r), device, _np_ptr(out)), "dpq_rotate")
    return out


def rotate_torch(vectors, rotation, out=None):
    """rotate on device tensors (dpq_rotate_device): enqueued on torch's current stream, no host round trip.  `out`
    must not be `vectors`."""
    import torch
    assert vectors.is_cuda and vectors.dtype == torch.float32 and vectors.is_contiguous() and vectors.dim() == 2
    assert rotation.is_cuda and rotation.dtype == torch.float32 and rotation.is_contiguous()
    n, D = vectors.shape
    assert tuple(rotation.shape) == (D, D), "rotation must be [D][D]"
    if out is None:
        out = torch.empty_like(vectors)
    if n == 0:
        return out
    with torch.cuda.device(vectors.device):
        stream = torch.cuda.current_stream(vectors.device).cuda_stream
        check(_lib.load().dpq_rotate_device(ctypes.c_void_p(vectors.data_ptr()), n, D, ctypes.c_void_p(rotation.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)), "dpq_rotate_device")
    return out


def cross_covariance(vectors, codes, codebook, device=0):
    """C = X^T Y in fp64, leaf-ordered (dpq_cross_covariance): Y is the reconstruction of `codes` under `codebook`,
    gathered on the GPU.  Returns float64 [D][D]."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    cb = np.ascontiguousarray(codebook, dtype=np.float32)
    assert v.ndim == 2 and c.ndim == 2 and cb.ndim == 3 and c.shape == (v.shape[0], cb.shape[0])
    M, K, Ds = cb.shape
    out = np.zeros((v.shape[1], v.shape[1]), dtype=np.float64)
    check(_lib.load().dpq_cross_covariance(_np_ptr(v), v.shape[0], v.shape[1], _np_ptr(c), _np_ptr(cb), M, K, Ds, device,
                                           _np_ptr(out)), "dpq_cross_covariance")
    return out


def procrustes(C):
    """The orthogonal polar factor U V^T of C = U S V^T (dpq_procrustes; host, fp64, one-sided Jacobi).  Returns
    (R float64 [D][D], degenerate bool); R is all zeros when degenerate."""
    c = np.ascontiguousarray(C, dtype=np.float64)
    assert c.ndim == 2 and c.shape[0] == c.shape[1]
    out = np.zeros_like(c)
    deg = _lib.c_i32(0)
    check(_lib.load().dpq_procrustes(_np_ptr(c), c.shape[0], _np_ptr(out), deg), "dpq_procrustes")
    return out, bool(deg.value)


def train_opq(vectors, M=8, K=256, outer_iters=8, init_iters=25, inner_iters=4, seed=0, start="rows", restarts=1,
              rotation=None, device=0):
    """OPQ on the GPU (dpq_opq_train): an orthogonal rotation learned together with the codebooks of the rotated space.
    rotation: a start [D][D] instead of the identity.  Returns (rotation float32 [D][D], codebook float32 [M][K][D / M],
    stats dict); the pair is the outer step with the lowest objective."""
    if start not in _TRAIN_STARTS:
        raise ValueError('start must be "rows" or "kmeans++"')
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert v.ndim == 2
    n, D = v.shape
    opts = _lib.OpqOpts(device=device, outer_iters=outer_iters, init_iters=init_iters, inner_iters=inner_iters, seed=seed,
                        init=_TRAIN_STARTS[start], restarts=restarts, use_initial_rotation=int(rotation is not None))
    if rotation is None:
        rot = np.zeros((D, D), dtype=np.float32)
    else:
        rot = np.array(rotation, dtype=np.float32, order="C")
        assert rot.shape == (D, D), "rotation must be [D][D]"
    cb = np.zeros((max(M, 1), max(K, 1), max(D // M, 1) if M >= 1 else 1), dtype=np.float32)
    st = _lib.OpqStats()
    check(lib.dpq_opq_train(_np_ptr(v), n, D, M, K, opts, _np_ptr(rot), _np_ptr(cb), st), "dpq_opq_train")
    stats = {k: getattr(st, k) for k, _ in st._fields_ if k not in ("objective", "rotation_residual", "reserved")}
    stats["objective"] = [st.objective[i] for i in range(st.outer_run + 1)]
    stats["rotation_residual"] = [st.rotation_residual[i] for i in range(st.outer_run)]
    return rot, cb, stats


def write_rotation(path, rotation):
    """The rotation file (dpq_write_rotation): .fvecs layout, D rows of D floats."""
    r = np.ascontiguousarray(rotation, dtype=np.float32)
    assert r.ndim == 2 and r.shape[0] == r.shape[1]
    check(_lib.load().dpq_write_rotation(path.encode(), _np_ptr(r), r.shape[0]), "dpq_write_rotation")


def read_rotation(path):
    """float32 [D][D] of a rotation file (dpq_read_rotation); a truncated or non-square file raises DpqError."""
    lib = _lib.load()
    D = _lib.c_i32()
    check(lib.dpq_read_rotation(path.encode(), D, None), "dpq_read_rotation")
    out = np.empty((D.value, D.value), dtype=np.float32)
    check(lib.dpq_read_rotation(path.encode(), D, _np_ptr(out)), "dpq_read_rotation")
    return out


def rotation_file_name(dataset_dir, M, K):
    import os
    return os.path.join(dataset_dir, "M%dK%drotation.fvecs" % (M, K))


def read_codes_plain(path, M):
    """PQTree::Read (pq_tree.cpp:1032-1081): uint8 [N][M]."""
    lib = _lib.load()
    n = _lib.c_i64()
    check(lib.dpq_read_codes_plain(path.encode(), M, n, None), "dpq_read_codes_plain")
    out = np.empty((n.value, M), dtype=np.uint8)
    check(lib.dpq_read_codes_plain(path.encode(), M, n, _np_ptr(out)), "dpq_read_codes_plain")
    return out


def read_codes_plain_ex(path, M, K=256, with_id=False):
    """PQTree::Read's other layouts (pq_tree.cpp:1050-1078): uint16 codes for K > 256, (code, int32 id) records with_id.
    Returns (codes [N][M] uint8 or uint16, ids int32 [N] or None)."""
    lib = _lib.load()
    n = _lib.c_i64()
    check(lib.dpq_read_codes_plain_ex(path.encode(), M, K, int(with_id), n, None, None), "dpq_read_codes_plain_ex")
    codes = np.empty((n.value, M), dtype=np.uint16 if K > 256 else np.uint8)
    ids = np.empty(n.value, dtype=np.int32) if with_id else None
    check(lib.dpq_read_codes_plain_ex(path.encode(), M, K, int(with_id), n, _np_ptr(codes), None if ids is None else _np_ptr(ids)),
          "dpq_read_codes_plain_ex")
    return codes, ids


def write_codes_plain(path, codes):
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    check(_lib.load().dpq_write_codes_plain(path.encode(), _np_ptr(c), c.shape[0], c.shape[1]), "dpq_write_codes_plain")


def read_qnode_ids(path, n_codes):
    """DFS position -> original vector id (QNode.vec_id) from a TreeNodesDFS file."""
    out = np.empty(n_codes, dtype=np.uint32)
    check(_lib.load().dpq_read_qnode_ids(path.encode(), n_codes, _np_ptr(out)), "dpq_read_qnode_ids")
    return out


def _apply_tuning(opts, tune):
    """dpq_open_opts' plan and tiling knobs by name (stream_max_queries, coarse_below, plan_ratios, boot_cap,
    boot_target, flags, batch_tile_nodes); 0 / absent = the measured default."""
    for name, value in tune.items():
        if name == "plan_ratios":
            vals = list(value) + [0, 0, 0]
            for i in range(3):
                opts.plan_ratios[i] = int(vals[i])
        elif name in ("stream_max_queries", "coarse_below", "boot_cap", "boot_target", "flags", "batch_tile_nodes"):
            v = int(value)
            if name == "stream_max_queries" and v > MAX_STREAM_QUERIES:
                raise ValueError("stream_max_queries above %d: the stream pass answers at most four queries per pass" % MAX_STREAM_QUERIES)
            if name == "boot_cap" and v != 0 and not 2048 <= v <= 16384:
                raise ValueError("boot_cap outside 2048..16384")
            setattr(opts, name, v)
        else:
            raise TypeError("unknown dpq_open_opts field %r" % name)
    return opts


# dpq_open_opts.flags (include/deltapq_amd.h DPQ_OPT_*)
OPT_NO_RELABEL, OPT_NO_FUSE_QUANTISE, OPT_NO_ASYNC_OVERLAP, OPT_BOOT_FULLSORT = 1, 2, 4, 8
OPT_NO_TIGHTEN, OPT_NO_STRANDS, OPT_FORCE_STRANDS, OPT_NO_STRAND1 = 16, 32, 64, 128
MAX_STREAM_QUERIES = 16   # a larger stream_max_queries would send a big batch through ceil(nq / 4) full passes over the index


class DeltaPQIndex:
    """One DTC index (or one shard) resident on one MI355X."""

    def __init__(self, handle):
        self._h = handle
        self._lib = _lib.load()

    @classmethod
    def open_file(cls, path, M=8, K=256, device=0, shard_rank=0, shard_count=1, chunks_per_segment=0,
                  cand_capacity=0, num_codes=0, bootstrap=0, batch_decode=0, **tune):
        """num_codes > 0: scan only the first num_codes codes (the reference's -N below the header's n_codes).
        bootstrap: 0 auto, 1 on, -1 off (dpq_open_opts.bootstrap).  batch_decode: 0 auto, 1 always decode once per batch
        into the plain-code scratch, -1 always decode inside the scan, n >= 2 scratch in tiles of n segments
        (dpq_open_opts.batch_decode)."""
        lib = _lib.load()
        opts = _apply_tuning(OpenOpts(device, shard_rank, shard_count, chunks_per_segment, cand_capacity, num_codes, bootstrap,
                                      batch_decode), tune)
        h = ctypes.c_void_p()
        check(lib.dpq_open_file(path.encode(), M, K, opts, h), "dpq_open_file")
        return cls(h)

    @classmethod
    def open_memory(cls, payload, n_codes, M=8, K=256, device=0, shard_rank=0, shard_count=1, chunks_per_segment=0,
                    cand_capacity=0, num_codes=0, bootstrap=0, global_offset=0, global_n_codes=0, batch_decode=0, **tune):
        """global_offset / global_n_codes: the payload is a self-contained part of a larger index (ids are
        reported as global_offset + local position; dpq_open_opts)."""
        lib = _lib.load()
        pl = np.ascontiguousarray(payload, dtype=np.uint8)
        opts = _apply_tuning(OpenOpts(device, shard_rank, shard_count, chunks_per_segment, cand_capacity, num_codes, bootstrap,
                                      batch_decode, global_offset, global_n_codes), tune)
        h = ctypes.c_void_p()
        check(lib.dpq_open_memory(_np_ptr(pl), pl.size, n_codes, M, K, opts, h), "dpq_open_memory")
        return cls(h)

    @classmethod
    def open_plain(cls, codes, K=256, device=0, shard_rank=0, shard_count=1, chunks_per_segment=0, cand_capacity=0,
                   num_codes=0, bootstrap=0, **tune):
        """Uncompressed comparator index (`-task pqscan`, h:2590-2678): raw codes, fp32-accumulated distances."""
        lib = _lib.load()
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        opts = _apply_tuning(OpenOpts(device, shard_rank, shard_count, chunks_per_segment, cand_capacity, num_codes, bootstrap), tune)
        h = ctypes.c_void_p()
        check(lib.dpq_open_plain_memory(_np_ptr(c), c.shape[0], c.shape[1], K, opts, h), "dpq_open_plain_memory")
        return cls(h)

    def set_codebook(self, codebook):
        cb = np.ascontiguousarray(codebook, dtype=np.float32)
        assert cb.ndim == 3
        check(self._lib.dpq_set_codebook(self._h, _np_ptr(cb), cb.shape[2]), "dpq_set_codebook")
        return self

    def info(self):
        i = Info()
        check(self._lib.dpq_get_info(self._h, i), "dpq_get_info")
        return i.as_dict()

    def query_batch(self, queries, top_k):
        """Host buffers in/out.  Returns (ids int32 [nq][k], dists float32 [nq][k])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        ids = np.empty((nq, top_k), dtype=np.int32)
        dists = np.empty((nq, top_k), dtype=np.float32)
        check(self._lib.dpq_query_batch(self._h, _np_ptr(q), nq, top_k, _np_ptr(ids), _np_ptr(dists)),
              "dpq_query_batch")
        return ids, dists

    def range_search(self, queries, radius):
        """Every code within `radius` of each query (dpq_range_search): d < radius, strictly.  `radius` is a scalar or one
        value per query.  Returns (lims int64 [nq + 1], ids int32 [lims[-1]], dists float32 [lims[-1]]); query i owns
        entries lims[i]:lims[i + 1], ascending by (distance, id)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        res = ctypes.c_void_p()
        check(self._lib.dpq_range_search(self._h, _np_ptr(q), nq, _np_ptr(r), res), "dpq_range_search")
        try:
            n = _lib.c_i32()
            pl, pi, pd = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            check(self._lib.dpq_range_result_get(res, n, pl, pi, pd), "dpq_range_result_get")
            lims = np.ctypeslib.as_array(ctypes.cast(pl, ctypes.POINTER(_lib.c_i64)), (n.value + 1,)).copy()
            total = int(lims[-1])
            ids = np.empty(total, dtype=np.int32)
            dists = np.empty(total, dtype=np.float32)
            if total:
                ctypes.memmove(ids.ctypes.data, pi.value, total * 4)
                ctypes.memmove(dists.ctypes.data, pd.value, total * 4)
            return lims, ids, dists
        finally:
            self._lib.dpq_range_result_free(res)

    def query_batch_filtered(self, queries, top_k, id_filter):
        """The top_k nearest codes among those `id_filter` (an IdFilter made on this index) allows
        (dpq_query_batch_filtered).  Returns (ids int32 [nq][k], dists float32 [nq][k]); rows are padded with -1 / +inf
        where fewer than top_k codes are allowed."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        ids = np.empty((nq, top_k), dtype=np.int32)
        dists = np.empty((nq, top_k), dtype=np.float32)
        check(self._lib.dpq_query_batch_filtered(self._h, IdFilter._handle(id_filter), _np_ptr(q), nq, top_k, _np_ptr(ids),
                                                 _np_ptr(dists)), "dpq_query_batch_filtered")
        return ids, dists

    def query_batch_filtered_torch(self, queries, top_k, id_filter, out_ids=None, out_dists=None):
        """query_batch_filtered on device tensors, synchronous on torch's current stream
        (dpq_query_batch_device_filtered)."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        check(self._lib.dpq_query_batch_device_filtered(self._h, IdFilter._handle(id_filter), ctypes.c_void_p(queries.data_ptr()),
                                                        nq, top_k, ctypes.c_void_p(out_ids.data_ptr()),
                                                        ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(stream)),
              "dpq_query_batch_device_filtered")
        return out_ids, out_dists

    # ---- search by distance tables, and inner product (include/deltapq_amd.h) ----

    def _tables(self, tables):
        """float32 [nq][M][K], C-contiguous, of one table [M][K] or a batch of them."""
        info = self.info()
        t = np.ascontiguousarray(tables, dtype=np.float32)
        if t.ndim == 2:
            t = t[None]
        assert t.ndim == 3 and t.shape[1:] == (info["M"], info["K"]), "tables must be [nq][M][K] of this index"
        return t

    def query_batch_tables(self, tables, top_k, id_filter=None):
        """query_batch[_filtered] with the caller's distance tables [nq][M][K] standing where the L2 tables of the
        queries stand (dpq_query_batch_tables); needs no codebook.  Entries: finite >= 0 or +inf."""
        t = self._tables(tables)
        nq = t.shape[0]
        ids = np.empty((nq, top_k), dtype=np.int32)
        dists = np.empty((nq, top_k), dtype=np.float32)
        f = IdFilter._handle(id_filter) if id_filter is not None else None
        check(self._lib.dpq_query_batch_tables(self._h, f, _np_ptr(t), nq, top_k, _np_ptr(ids), _np_ptr(dists)),
              "dpq_query_batch_tables")
        return ids, dists

    def query_batch_tables_torch(self, tables, top_k, id_filter=None, out_ids=None, out_dists=None):
        """query_batch_tables on device tensors ([nq][M][K] float32, contiguous), synchronous on torch's current stream
        (dpq_query_batch_device_tables)."""
        import torch
        assert tables.is_cuda and tables.dtype == torch.float32 and tables.is_contiguous() and tables.dim() == 3
        nq = tables.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=tables.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=tables.device)
        stream = torch.cuda.current_stream(tables.device).cuda_stream
        f = IdFilter._handle(id_filter) if id_filter is not None else None
        check(self._lib.dpq_query_batch_device_tables(self._h, f, ctypes.c_void_p(tables.data_ptr()), nq, top_k,
                                                      ctypes.c_void_p(out_ids.data_ptr()),
                                                      ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(stream)),
              "dpq_query_batch_device_tables")
        return out_ids, out_dists

    def range_search_tables(self, tables, radius, id_filter=None):
        """range_search with the caller's distance tables (dpq_range_search_tables).  Range search takes no filter:
        id_filter must be None."""
        if id_filter is not None:
            raise ValueError("range_search_tables takes no id_filter (dpq_range_search has no filtered form)")
        t = self._tables(tables)
        nq = t.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        res = ctypes.c_void_p()
        check(self._lib.dpq_range_search_tables(self._h, _np_ptr(t), nq, _np_ptr(r), res), "dpq_range_search_tables")
        return _range_result(self._lib, res)

    def ip_tables(self, queries, id_filter=None):
        """(tables float32 [nq][M][K], bias float32 [nq]) of the inner-product rule (dpq_ip_tables): the tables
        query_batch_tables takes, gaps to each sub-space's best centroid.  A filter has no part in them: id_filter must
        be None."""
        if id_filter is not None:
            raise ValueError("ip_tables takes no id_filter: the tables depend on the queries and the codebook only")
        q =np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        info = self.info()
        nq = q.shape[0]
        tables = np.empty((nq, info["M"], info["K"]), dtype=np.float32)
        bias = np.empty(nq, dtype=np.float32)
        check(self._lib.dpq_ip_tables(self._h, _np_ptr(q), nq, _np_ptr(tables), _np_ptr(bias)), "dpq_ip_tables")
        return tables, bias

    def ip_tables_torch(self, queries, out_tables=None, out_bias=None):
        """ip_tables on device tensors, enqueued on torch's current stream and nothing else (dpq_ip_tables_device)."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        info = self.info()
        nq = queries.shape[0]
        if out_tables is None:
            out_tables = torch.empty((nq, info["M"], info["K"]), dtype=torch.float32, device=queries.device)
        if out_bias is None:
            out_bias = torch.empty((nq,), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        check(self._lib.dpq_ip_tables_device(self._h, ctypes.c_void_p(queries.data_ptr()), nq,
                                             ctypes.c_void_p(out_tables.data_ptr()), ctypes.c_void_p(out_bias.data_ptr()),
                                             ctypes.c_void_p(stream)), "dpq_ip_tables_device")
        return out_tables, out_bias

    def query_batch_ip(self, queries, top_k, id_filter=None):
        """The top_k codes of the largest approximate inner product with each query (dpq_query_batch_ip).  Returns
        (ids int32 [nq][k], scores float32 [nq][k] descending, gaps float32 [nq][k], bias float32 [nq]); padding rows
        are -1 / -inf / +inf."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        ids = np.empty((nq, top_k), dtype=np.int32)
        scores = np.empty((nq, top_k), dtype=np.float32)
        gaps = np.empty((nq, top_k), dtype=np.float32)
        bias = np.empty(nq, dtype=np.float32)
        f = IdFilter._handle(id_filter) if id_filter is not None else None
        check(self._lib.dpq_query_batch_ip(self._h, f, _np_ptr(q), nq, top_k, _np_ptr(ids), _np_ptr(scores), _np_ptr(gaps),
                                           _np_ptr(bias)), "dpq_query_batch_ip")
        return ids, scores, gaps, bias

    def query_batch_ip_torch(self, queries, top_k, id_filter=None, out_ids=None, out_scores=None, out_gaps=None,
                             out_bias=None):
        """query_batch_ip on device tensors, synchronous on torch's current stream (dpq_query_batch_device_ip).  Returns
        (ids, scores); gaps and bias are written where out_gaps / out_bias are given."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_scores is None:
            out_scores = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        f = IdFilter._handle(id_filter) if id_filter is not None else None
        opt = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        check(self._lib.dpq_query_batch_device_ip(self._h, f, ctypes.c_void_p(queries.data_ptr()), nq, top_k,
                                                  ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_scores.data_ptr()),
                                                  opt(out_gaps), opt(out_bias), ctypes.c_void_p(stream)),
              "dpq_query_batch_device_ip")
        return out_ids, out_scores

    # ---- candidate search: PQ distances and top-k over each query's own ids (include/deltapq_amd.h) ----

    @staticmethod
    def _cand(cand_ids, nq):
        """int32 [nq][n_cand], C-contiguous; ragged lists come padded with -1."""
        c = np.ascontiguousarray(cand_ids, dtype=np.int32)
        if c.ndim == 1:
            c = c[None, :]
        assert c.ndim == 2 and c.shape[0] == nq, "cand_ids must be [nq][n_cand]"
        return c

    def _candidate_search(self, fn, name, rows, cand_ids, top_k):
        c = self._cand(cand_ids, rows.shape[0])
        nq = rows.shape[0]
        ids = np.empty((nq, top_k), dtype=np.int32)
        dists = np.empty((nq, top_k), dtype=np.float32)
        check(fn(self._h, _np_ptr(rows), nq, _np_ptr(c), c.shape[1], top_k, _np_ptr(ids), _np_ptr(dists)), name)
        return ids, dists

    def candidate_search(self, queries, cand_ids, top_k):
        """The best top_k of each query's own candidates by PQ distance (dpq_candidate_search): cand_ids int32
        [nq][n_cand] of reported ids, -1 = padding, another shard's ids are skipped.  Returns (ids int32 [nq][k], dists
        float32 [nq][k]), the distances query_batch reports for those ids, padded with -1 / +inf."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        return self._candidate_search(self._lib.dpq_candidate_search, "dpq_candidate_search", q, cand_ids, top_k)

    def candidate_search_tables(self, tables, cand_ids, top_k):
        """candidate_search with the caller's distance tables [nq][M][K] (dpq_candidate_search_tables); needs no
        codebook."""
        return self._candidate_search(self._lib.dpq_candidate_search_tables, "dpq_candidate_search_tables",
                                      self._tables(tables), cand_ids, top_k)

    def candidate_distances(self, queries, cand_ids):
        """float32 [nq][n_cand]: the PQ distance of cand_ids[q][j] to query q, in place (dpq_candidate_distances); NaN
        where the entry is padding or another shard's id."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        c = self._cand(cand_ids, q.shape[0])
        dists = np.empty(c.shape, dtype=np.float32)
        check(self._lib.dpq_candidate_distances(self._h, _np_ptr(q), q.shape[0], _np_ptr(c), c.shape[1], _np_ptr(dists)),
              "dpq_candidate_distances")
        return dists

    def _candidate_search_torch(self, fn, name, rows, cand_ids, top_k, out_ids, out_dists):
        import torch
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()
        assert cand_ids.is_cuda and cand_ids.dtype == torch.int32 and cand_ids.is_contiguous() and cand_ids.dim() == 2
        nq = rows.shape[0]
        assert cand_ids.shape[0] == nq
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=rows.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=rows.device)
        stream = torch.cuda.current_stream(rows.device).cuda_stream
        check(fn(self._h, ctypes.c_void_p(rows.data_ptr()), nq, ctypes.c_void_p(cand_ids.data_ptr()), cand_ids.shape[1], top_k,
                 ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(stream)), name)
        return out_ids, out_dists

    def candidate_search_torch(self, queries, cand_ids, top_k, out_ids=None, out_dists=None):
        """candidate_search on device tensors, synchronous on torch's current stream (dpq_candidate_search_device)."""
        return self._candidate_search_torch(self._lib.dpq_candidate_search_device, "dpq_candidate_search_device", queries,
                                            cand_ids, top_k, out_ids, out_dists)

    def candidate_search_tables_torch(self, tables, cand_ids, top_k, out_ids=None, out_dists=None):
        """candidate_search_tables on device tensors ([nq][M][K] float32), synchronous on torch's current stream
        (dpq_candidate_search_device_tables)."""
        assert tables.dim() == 3
        return self._candidate_search_torch(self._lib.dpq_candidate_search_device_tables,
                                            "dpq_candidate_search_device_tables", tables, cand_ids, top_k, out_ids, out_dists)

    def candidate_distances_torch(self, queries, cand_ids, out=None):
        """candidate_distances on device tensors, synchronous on torch's current stream
        (dpq_candidate_distances_device)."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        assert cand_ids.is_cuda and cand_ids.dtype == torch.int32 and cand_ids.is_contiguous() and cand_ids.dim() == 2
        nq = queries.shape[0]
        assert cand_ids.shape[0] == nq
        if out is None:
            out = torch.empty(tuple(cand_ids.shape), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        check(self._lib.dpq_candidate_distances_device(self._h, ctypes.c_void_p(queries.data_ptr()), nq,
                                                       ctypes.c_void_p(cand_ids.data_ptr()), cand_ids.shape[1],
                                                       ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)),
              "dpq_candidate_distances_device")
        return out

    def set_vec_ids(self, vec_id):
        """The original vector id of every node this handle holds (dpq_set_vec_ids): `vec_id` is the handle's local
        slice, uint32 [node_hi - node_lo], of the builder's DFS position -> vector id array.  Kept on the device for
        IdFilter.from_vec_* only; searches keep reporting DFS positions."""
        v = np.ascontiguousarray(vec_id, dtype=np.uint32).ravel()
        check(self._lib.dpq_set_vec_ids(self._h, _np_ptr(v) if v.size else None, v.size), "dpq_set_vec_ids")
        return self

    def _lookup_ids(self, ids):
        return np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))

    def get_codes(self, ids):
        """The codes of reported ids (dpq_get_codes), uint8 [n][M].  An id is what a search reports; a negative id is
        padding and gives a zero row; an id that names no node of this handle raises DpqError (DPQ_ERR_ARG)."""
        i = self._lookup_ids(ids)
        out = np.empty((i.size, self.info()["M"]), dtype=np.uint8)
        check(self._lib.dpq_get_codes(self._h, _np_ptr(i), i.size, _np_ptr(out)), "dpq_get_codes")
        return out

    def reconstruct(self, ids):
        """The codebook's approximation of reported ids (dpq_reconstruct), float32 [n][M * Ds]: row i is the
        concatenation of codebook[m, code_i[m]].  A negative id gives a row of NaNs."""
        i = self._lookup_ids(ids)
        inf = self.info()
        out = np.empty((i.size, inf["M"] * inf["Ds"]), dtype=np.float32)
        check(self._lib.dpq_reconstruct(self._h, _np_ptr(i), i.size, _np_ptr(out)), "dpq_reconstruct")
        return out

    def decode_range(self, first=None, count=None):
        """The handle's codes for POSITIONS [first, first + count) in DFS order (dpq_decode_range), uint8 [count][M];
        by default everything the handle holds, info()["node_lo"] .. info()["node_hi"]."""
        inf = self.info()
        if first is None:
            first = inf["node_lo"]
        if count is None:
            count = inf["node_hi"] - first
        out = np.empty((max(int(count), 0), inf["M"]), dtype=np.uint8)
        check(self._lib.dpq_decode_range(self._h, first, count, _np_ptr(out)), "dpq_decode_range")
        return out

    def get_codes_torch(self, ids, out=None):
        """get_codes on device tensors, synchronous on torch's current stream (dpq_get_codes_device): `ids` int32 [n]
        on the index's GPU; returns uint8 [n][M] there."""
        import torch
        assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous()
        n = ids.numel()
        if out is None:
            out = torch.empty((n, self.info()["M"]), dtype=torch.uint8, device=ids.device)
        if n == 0:                      # (an empty tensor has no storage: nothing to hand to the library)
            return out
        stream = torch.cuda.current_stream(ids.device).cuda_stream
        check(self._lib.dpq_get_codes_device(self._h, ctypes.c_void_p(ids.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                             ctypes.c_void_p(stream)), "dpq_get_codes_device")
        return out

    def reconstruct_torch(self, ids, out=None):
        """reconstruct on device tensors, synchronous on torch's current stream (dpq_reconstruct_device): returns
        float32 [n][M * Ds] on the index's GPU."""
        import torch
        assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous()
        n = ids.numel()
        if out is None:
            inf = self.info()
            out = torch.empty((n, inf["M"] * inf["Ds"]), dtype=torch.float32, device=ids.device)
        if n == 0:
            return out
        stream = torch.cuda.current_stream(ids.device).cuda_stream
        check(self._lib.dpq_reconstruct_device(self._h, ctypes.c_void_p(ids.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                               ctypes.c_void_p(stream)), "dpq_reconstruct_device")
        return out

    def query_batch_host_async(self, queries, top_k, ids, dists):
        """dpq_query_batch_host_async: host arrays in and out, enqueued only -- up to four batches in flight, queries up and
        results down beside the kernels.  `queries` (float32 [nq][D], C-contiguous), `ids` (int32 [nq][k]) and `dists`
        (float32 [nq][k]) belong to the library until finish(); pin them (pin_host) for the copies to overlap."""
        assert queries.dtype == np.float32 and queries.flags.c_contiguous and ids.dtype == np.int32 and dists.dtype == np.float32
        assert ids.flags.c_contiguous and dists.flags.c_contiguous and ids.shape == dists.shape == (queries.shape[0], top_k)
        check(self._lib.dpq_query_batch_host_async(self._h, _np_ptr(queries), queries.shape[0], top_k, _np_ptr(ids), _np_ptr(dists)),
              "dpq_query_batch_host_async")

    def query_batch_torch(self, queries, top_k, out_ids=None, out_dists=None, wait=True, ordered=False):
        """Device tensors in/out on torch's current stream (no host copies).  wait=False
        (dpq_query_batch_device_async) only enqueues the batch: keep the tensors alive and do
        not read the results before finish().  wait=False, ordered=True (dpq_query_batch_device_ordered):
        enqueued on the current stream itself, later work on that stream sees the result unless
        finish() reports a rerun."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        fn = self._lib.dpq_query_batch_device if wait else (
            self._lib.dpq_query_batch_device_ordered if ordered else self._lib.dpq_query_batch_device_async)
        check(fn(self._h, ctypes.c_void_p(queries.data_ptr()), nq, top_k, ctypes.c_void_p(out_ids.data_ptr()),
                 ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(stream)),
              "dpq_query_batch_device" if wait else "dpq_query_batch_device_async")
        return out_ids, out_dists

    def finish(self):
        """Wait for the batches enqueued with wait=False and settle their overflow checks (dpq_finish).
        Returns the number of batches that had to be answered again."""
        n = _lib.c_i32()
        check(self._lib.dpq_finish_count(self._h, n), "dpq_finish_count")
        return n.value

    def profile_enable(self, on=True):
        check(self._lib.dpq_profile_enable(self._h, int(on)), "dpq_profile_enable")

    def profile_reset(self):
        check(self._lib.dpq_profile_reset(self._h), "dpq_profile_reset")

    def profile_read(self):
        p = Profile()
        check(self._lib.dpq_profile_read(self._h, p), "dpq_profile_read")
        return p.as_dict()

    def close(self):
        if self._h is not None:
            self._lib.dpq_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RotatedIndex:
    """An index over codes of ROTATED vectors (OPQ) that takes raw queries: every search rotates its queries on the
    index's GPU (dpq_rotate_device, into a buffer this object owns) and then calls the unchanged method of the index
    it wraps.  The rotation stays on the device.  Everything else (info, get_codes, ...) passes through."""

    def __init__(self, index, rotation):
        import torch
        r = np.ascontiguousarray(rotation, dtype=np.float32)
        assert r.ndim == 2 and r.shape[0] == r.shape[1], "rotation must be [D][D]"
        self.index = index
        self._device = torch.device("cuda", index.info()["device"])
        self._rot = torch.from_numpy(r).to(self._device)
        self._buf = None

    def _rotated(self, queries):
        """Device tensor [nq][D] of the rotated queries; valid until the next call."""
        import torch
        if isinstance(queries, torch.Tensor):
            q = queries
            assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()
        else:
            h = np.ascontiguousarray(queries, dtype=np.float32)
            if h.ndim == 1:
                h = h[None, :]
            q = torch.from_numpy(h).to(self._device)
        if self._buf is None or self._buf.shape[0] < q.shape[0]:
            self._buf = torch.empty((q.shape[0], self._rot.shape[0]), dtype=torch.float32, device=self._device)
        return rotate_torch(q, self._rot, out=self._buf[:q.shape[0]])

    def _rotated_host(self, queries):
        return self._rotated(queries).cpu().numpy()

    def query_batch(self, queries, top_k):
        return self.index.query_batch(self._rotated_host(queries), top_k)

    def query_batch_filtered(self, queries, top_k, id_filter):
        return self.index.query_batch_filtered(self._rotated_host(queries), top_k, id_filter)

    def range_search(self, queries, radius):
        return self.index.range_search(self._rotated_host(queries), radius)

    def query_batch_torch(self, queries, top_k, **kw):
        return self.index.query_batch_torch(self._rotated(queries), top_k, **kw)

    def query_batch_ip(self, queries, top_k, id_filter=None):
        """An orthogonal rotation leaves inner products alone: rotate the queries, then the index's own call."""
        return self.index.query_batch_ip(self._rotated_host(queries), top_k, id_filter=id_filter)

    def candidate_search(self, queries, cand_ids, top_k):
        return self.index.candidate_search(self._rotated_host(queries), cand_ids, top_k)

    def candidate_distances(self, queries, cand_ids):
        return self.index.candidate_distances(self._rotated_host(queries), cand_ids)

    def candidate_search_torch(self, queries, cand_ids, top_k, **kw):
        return self.index.candidate_search_torch(self._rotated(queries), cand_ids, top_k, **kw)

    def candidate_distances_torch(self, queries, cand_ids, **kw):
        return self.index.candidate_distances_torch(self._rotated(queries), cand_ids, **kw)

    def __getattr__(self, name):
        if name == "index":      # (not set yet: __init__ failed early)
            raise AttributeError(name)
        return getattr(self.index, name)


class IdFilter:
    """A filter of DeltaPQIndex.query_batch_filtered (dpq_filter): the set of reported ids a search may return, uploaded
    once to the index's device and used by any number of calls on that index.  Bit i of the bitmap is bit (i & 31) of
    word i >> 5; ids at or beyond n_bits are not allowed."""

    def __init__(self, index, words, n_bits):
        self._lib = _lib.load()
        self._h = None
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if n_bits < 0 or w.size < (n_bits + 31) // 32:
            raise ValueError("words must hold n_bits >= 0 bits")
        h = ctypes.c_void_p()
        check(self._lib.dpq_filter_create(index._h, _np_ptr(w) if w.size else None, int(n_bits), h), "dpq_filter_create")
        self._h = h
        self._index = index

    @classmethod
    def _wrap(cls, index, handle):
        """An IdFilter around a dpq_filter the library has already made on `index`."""
        f = cls.__new__(cls)
        f._lib = index._lib
        f._h = handle
        f._index = index
        return f

    @classmethod
    def _create(cls, index, name, *args):
        """One of the dpq_filter_create_* constructors: fn(index, *args, &out)."""
        h = ctypes.c_void_p()
        check(getattr(index._lib, name)(index._h, *args, h), name)
        return cls._wrap(index, h)

    @staticmethod
    def pack_mask(mask):
        """bool [n] -> (uint32 words [(n + 31) // 32], n): little-endian bits."""
        m = np.ascontiguousarray(mask, dtype=bool).ravel()
        n = m.size
        b = np.packbits(m, bitorder="little")
        b = np.concatenate([b, np.zeros((-b.size) % 4, dtype=np.uint8)])
        return b.view("<u4").astype(np.uint32), n

    @staticmethod
    def pack_ids(ids, n_bits=None):
        """allowed ids -> (words, n_bits); n_bits defaults to max(ids) + 1."""
        a = np.asarray(ids, dtype=np.int64).ravel()
        if n_bits is None:
            n_bits = int(a.max()) + 1 if a.size else 0
        if a.size and (a.min() < 0 or a.max() >= n_bits):
            raise ValueError("ids must lie in [0, n_bits)")
        m = np.zeros(n_bits, dtype=bool)
        m[a] = True
        return IdFilter.pack_mask(m)

    @staticmethod
    def unpack(words, n_bits):
        """(words, n_bits) -> bool [n_bits]."""
        w = np.ascontiguousarray(words, dtype=np.uint32).astype("<u4")
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:n_bits].astype(bool)

    @classmethod
    def from_mask(cls, index, mask):
        """mask[i]: whether reported id i is allowed."""
        return cls(index, *cls.pack_mask(mask))

    @classmethod
    def from_ids(cls, index, ids, n_bits=None, invert=False):
        """The listed reported ids (invert=True: every code of the index except them).  With `n_bits` the list is packed
        into a bitmap on the host (ids must lie in [0, n_bits)); without, or with invert, it goes to the GPU as it is
        (dpq_filter_create_ids): negative ids are padding, ids of other shards are skipped."""
        if not invert and n_bits is not None:
            return cls(index, *cls.pack_ids(ids, n_bits))
        if n_bits is not None:
            raise ValueError("a deny-list takes no n_bits: it allows every code of the index but the listed ones")
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        return cls._create(index, "dpq_filter_create_ids", _np_ptr(a) if a.size else None, a.size, int(bool(invert)))

    @classmethod
    def from_range(cls, index, lo, hi):
        """Reported ids in [lo, hi) (dpq_filter_create_range)."""
        return cls._create(index, "dpq_filter_create_range", int(lo), int(hi))

    @classmethod
    def from_vec_mask(cls, index, mask):
        """mask[v]: whether ORIGINAL vector id v is allowed (dpq_filter_create_vec; index.set_vec_ids first)."""
        w, n = cls.pack_mask(mask)
        return cls._create(index, "dpq_filter_create_vec", _np_ptr(w) if w.size else None, n)

    @classmethod
    def from_vec_ids(cls, index, ids, n_bits=None):
        """The listed ORIGINAL vector ids (index.set_vec_ids first)."""
        w, n = cls.pack_ids(ids, n_bits)
        return cls._create(index, "dpq_filter_create_vec", _np_ptr(w) if w.size else None, n)

    # -- torch forms: CUDA tensors on the index's GPU, torch's current stream; nothing but the count goes to the host

    @staticmethod
    def _torch_words(index, n_bits, fill, *args):
        """A device bitmap of n_bits bits, packed by one of the dpq_bitmap_from_*_device helpers: (tensor, pointer, stream)."""
        import torch
        dev = args[0].device
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        words = torch.empty(((n_bits + 31) // 32,), dtype=torch.int32, device=dev)
        ptrs = [ctypes.c_void_p(t.data_ptr()) if t.numel() else None for t in args]
        wp = ctypes.c_void_p(words.data_ptr()) if words.numel() else None
        if fill == "mask":
            check(index._lib.dpq_bitmap_from_mask_device(ptrs[0], args[0].numel(), wp, dev.index or 0, stream),
                  "dpq_bitmap_from_mask_device")
        else:
            check(index._lib.dpq_bitmap_from_ids_device(ptrs[0], args[0].numel(), n_bits, wp, dev.index or 0, stream),
                  "dpq_bitmap_from_ids_device")
        return words, wp, stream

    @staticmethod
    def _torch_arg(t, dtype):
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous()
        return t.reshape(-1)

    @classmethod
    def from_mask_torch(cls, index, mask):
        """from_mask for a bool CUDA tensor over reported ids."""
        import torch
        m = cls._torch_arg(mask, torch.bool)
        words, wp, stream = cls._torch_words(index, m.numel(), "mask", m)
        return cls._create(index, "dpq_filter_create_device", wp, m.numel(), stream)

    @classmethod
    def from_ids_torch(cls, index, ids, invert=False):
        """from_ids for an int32 CUDA tensor of reported ids (dpq_filter_create_ids_device)."""
        import torch
        i = cls._torch_arg(ids, torch.int32)
        stream = ctypes.c_void_p(torch.cuda.current_stream(i.device).cuda_stream)
        return cls._create(index, "dpq_filter_create_ids_device", ctypes.c_void_p(i.data_ptr()) if i.numel() else None,
                           i.numel(), int(bool(invert)), stream)

    @classmethod
    def from_vec_mask_torch(cls, index, mask):
        """from_vec_mask for a bool CUDA tensor over ORIGINAL vector ids."""
        import torch
        m = cls._torch_arg(mask, torch.bool)
        words, wp, stream = cls._torch_words(index, m.numel(), "mask", m)
        return cls._create(index, "dpq_filter_create_vec_device", wp, m.numel(), stream)

    @classmethod
    def from_vec_ids_torch(cls, index, ids, n_bits):
        """from_vec_ids for an int32 CUDA tensor of ORIGINAL vector ids below n_bits (ids outside [0, n_bits) are skipped)."""
        import torch
        i = cls._torch_arg(ids, torch.int32)
        words, wp, stream = cls._torch_words(index, int(n_bits), "ids", i)
        return cls._create(index, "dpq_filter_create_vec_device", wp, int(n_bits), stream)

    # -- algebra and read-back

    def _combine(self, op, other):
        if other is not None and not isinstance(other, IdFilter):
            return NotImplemented
        return IdFilter._create(self._index, "dpq_filter_combine", op, self._h, None if other is None else other._h)

    def __and__(self, other):
        return self._combine(0, other)

    def __or__(self, other):
        return self._combine(1, other)

    def __sub__(self, other):
        """The codes this filter allows and `other` does not."""
        return self._combine(2, other)

    def __xor__(self, other):
        return self._combine(3, other)

    def __invert__(self):
        """Every code of the index this filter does not allow."""
        return self._combine(4, None)

    def to_mask(self, n_bits):
        """bool [n_bits] over reported ids: whether the filter allows the code its index reports under that id
        (dpq_filter_to_bitmap); ids that name no code of the index are False."""
        n_bits = int(n_bits)
        w = np.zeros((n_bits + 31) // 32, dtype=np.uint32)
        check(self._lib.dpq_filter_to_bitmap(self._h, _np_ptr(w) if w.size else None, n_bits), "dpq_filter_to_bitmap")
        return IdFilter.unpack(w, n_bits)

    @staticmethod
    def _handle(f):
        if not isinstance(f, IdFilter):
            raise TypeError("id_filter must be an IdFilter")
        return f._h

    @property
    def n_allowed(self):
        """Nodes of its index the filter allows."""
        n = _lib.c_i64()
        check(self._lib.dpq_filter_count(self._h, n), "dpq_filter_count")
        return n.value

    def close(self):
        if self._h is not None:
            self._lib.dpq_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def train_ivf_centroids(vectors, nlist, max_iters=25, seed=0, init=None, device=0):
    """The coarse quantiser of an IVF, learned on the GPU (dpq_ivf_train, include/deltapq_amd.h "IVF training"): Lloyd's
    rounds over whole vectors under the exact search's arithmetic.  init: a start [nlist][D] instead of the seeded rows.
    Returns (centroids float32 [nlist][D], stats dict)."""
    lib = _lib.load()
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert v.ndim == 2
    n, D = v.shape
    opts = _lib.IvfTrainOpts(device=device, max_iters=max_iters, seed=seed, use_initial=int(init is not None))
    if init is None:
        c = np.zeros((max(int(nlist), 1), D), dtype=np.float32)
    else:
        c = np.array(init, dtype=np.float32, order="C")
        assert c.shape == (nlist, D), "init must be [nlist][D]"
    st = _lib.IvfTrainStats()
    check(lib.dpq_ivf_train(_np_ptr(v), n, D, int(nlist), opts, _np_ptr(c), st), "dpq_ivf_train")
    stats = {k: getattr(st, k) for k, _ in st._fields_ if k != "distortion"}
    stats["distortion"] = [st.distortion[i] for i in range(st.iters_run)]
    return c, stats


def ivf_assign(centroids, vectors, device=0):
    """The nearest centroid of every vector, the lowest list at a tie (dpq_ivf_assign): (labels int32 [n], dists float32
    [n]), host arrays."""
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert c.ndim == 2 and v.ndim == 2 and c.shape[1] == v.shape[1], "centroids [nlist][D], vectors [n][D]"
    labels = np.empty(v.shape[0], dtype=np.int32)
    dists = np.empty(v.shape[0], dtype=np.float32)
    check(_lib.load().dpq_ivf_assign(_np_ptr(c), c.shape[0], c.shape[1], _np_ptr(v), v.shape[0], device, _np_ptr(labels),
                                     _np_ptr(dists)), "dpq_ivf_assign")
    return labels, dists


def ivf_assign_torch(centroids, vectors, out_labels=None, out_dists=None):
    """ivf_assign on device tensors (dpq_ivf_assign_device): enqueued on torch's current stream, no allocation by the
    library, no host round trip.  D must be a multiple of 4."""
    import torch
    for t in (centroids, vectors):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2
    n, D = vectors.shape
    assert centroids.shape[1] == D and centroids.device == vectors.device
    if out_labels is None:
        out_labels = torch.empty(n, dtype=torch.int32, device=vectors.device)
    if out_dists is None:
        out_dists = torch.empty(n, dtype=torch.float32, device=vectors.device)
    with torch.cuda.device(vectors.device):
        stream = torch.cuda.current_stream(vectors.device).cuda_stream
        check(_lib.load().dpq_ivf_assign_device(ctypes.c_void_p(centroids.data_ptr()), centroids.shape[0], D,
                                                ctypes.c_void_p(vectors.data_ptr()), n, ctypes.c_void_p(out_labels.data_ptr()),
                                                ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(stream)),
              "dpq_ivf_assign_device")
    return out_labels, out_dists


def write_vecs(path, vectors):
    """float32 [n][D] as an .fvecs file (dpq_write_vecs): read_vecs gives the same bits."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    assert v.ndim == 2
    check(_lib.load().dpq_write_vecs(path.encode(), _np_ptr(v), v.shape[0], v.shape[1]), "dpq_write_vecs")


class IVF:
    """Inverted lists over the nodes of one DeltaPQIndex (dpq_ivf, include/deltapq_amd.h "IVF search"): a query scans only
    the lists it probes.  Keeps its index alive; close it (or leave its `with` block) before the index is closed."""

    def __init__(self, index, handle):
        self._lib = index._lib
        self._index = index
        self._h = handle

    @classmethod
    def build(cls, index, centroids):
        """Lists by the nearest centroid of every node's reconstruction (dpq_ivf_build); centroids float32
        [nlist][M * Ds], kept for probe() and search()."""
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        assert c.ndim == 2, "centroids must be [nlist][M * Ds]"
        h = ctypes.c_void_p()
        check(index._lib.dpq_ivf_build(index._h, _np_ptr(c), c.shape[0], h), "dpq_ivf_build")
        return cls(index, h)

    @classmethod
    def from_labels(cls, index, labels, nlist, centroids=None):
        """Lists from labels (dpq_ivf_create; a CUDA int32 tensor: dpq_ivf_create_device on torch's current stream):
        labels[l] is the list of the index's local node l, -1 puts it in no list.  `centroids`: see set_centroids."""
        h = ctypes.c_void_p()
        if isinstance(labels, np.ndarray) or not hasattr(labels, "data_ptr"):
            a = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).ravel())
            check(index._lib.dpq_ivf_create(index._h, _np_ptr(a), a.size, int(nlist), h), "dpq_ivf_create")
        else:
            import torch
            assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous()
            stream = ctypes.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)
            check(index._lib.dpq_ivf_create_device(index._h, ctypes.c_void_p(labels.data_ptr()), labels.numel(), int(nlist),
                                                   stream, h), "dpq_ivf_create_device")
        ivf = cls(index, h)
        if centroids is not None:
            ivf.set_centroids(centroids)
        return ivf

    @classmethod
    def train(cls, index, vectors, vec_id, nlist, **opts):
        """End to end, as FAISS trains and fills an IndexIVF: train_ivf_centroids on the original `vectors` (**opts:
        max_iters, seed, init, device), ivf_assign of the same vectors, local node l into the list of its vector
        vec_id[l] (what set_vec_ids takes), the centroids kept for probe() and search()."""
        centroids, _ = train_ivf_centroids(vectors, nlist, **opts)
        vec_labels, _ = ivf_assign(centroids, vectors, device=opts.get("device", 0))
        labels = vec_labels[np.asarray(vec_id, dtype=np.int64)]
        return cls.from_labels(index, labels, nlist, centroids=centroids)

    def set_centroids(self, centroids):
        """Attaches centroids float32 [nlist][M * Ds] to lists made from labels (dpq_ivf_set_centroids)."""
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        assert c.ndim == 2, "centroids must be [nlist][M * Ds]"
        check(self._lib.dpq_ivf_set_centroids(self._h, _np_ptr(c), c.shape[0]), "dpq_ivf_set_centroids")
        return self

    def info(self):
        s = _lib.IvfStats()
        check(self._lib.dpq_ivf_get_info(self._h, s), "dpq_ivf_get_info")
        return s.as_dict()

    def lists(self):
        """(offsets int64 [nlist + 1], ids int32 [n_assigned]): list l holds ids[offsets[l]:offsets[l + 1]], the reported
        ids of its nodes, ascending (dpq_ivf_get)."""
        inf = self.info()
        offsets = np.empty(inf["nlist"] + 1, dtype=np.int64)
        ids = np.empty(inf["n_assigned"], dtype=np.int32)
        check(self._lib.dpq_ivf_get(self._h, _np_ptr(offsets), _np_ptr(ids) if ids.size else None), "dpq_ivf_get")
        return offsets, ids

    @staticmethod
    def _queries(queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        return q[None, :] if q.ndim == 1 else q

    def probe(self, queries, nprobe):
        """(lists int32 [nq][nprobe], dists float32 [nq][nprobe]): each query's nprobe nearest centroids by (exact L2
        distance, list number) (dpq_ivf_probe)."""
        q = self._queries(queries)
        lists = np.empty((q.shape[0], nprobe), dtype=np.int32)
        dists = np.empty((q.shape[0], nprobe), dtype=np.float32)
        check(self._lib.dpq_ivf_probe(self._h, _np_ptr(q), q.shape[0], nprobe, _np_ptr(lists), _np_ptr(dists)), "dpq_ivf_probe")
        return lists, dists

    @staticmethod
    def _probes(probes, nq):
        p = np.ascontiguousarray(probes, dtype=np.int32)
        if p.ndim == 1:
            p = p[None, :]
        assert p.ndim == 2 and p.shape[0] == nq, "probes must be [nq][nprobe]"
        return p

    @staticmethod
    def _filter(id_filter):
        return IdFilter._handle(id_filter) if id_filter is not None else None

    def search(self, queries, nprobe, top_k, id_filter=None):
        """The top_k nearest codes of the nprobe lists nearest to each query (dpq_ivf_search).  Returns (ids int32
        [nq][k], dists float32 [nq][k]), the distances query_batch reports for those ids, padded with -1 / +inf.
        `id_filter` (an IdFilter made on this IVF's index): only the codes it allows (dpq_ivf_search_filtered)."""
        q = self._queries(queries)
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        if id_filter is None:
            check(self._lib.dpq_ivf_search(self._h, _np_ptr(q), q.shape[0], nprobe, top_k, _np_ptr(ids), _np_ptr(dists)),
                  "dpq_ivf_search")
        else:
            check(self._lib.dpq_ivf_search_filtered(self._h, IdFilter._handle(id_filter), _np_ptr(q), q.shape[0], nprobe, top_k,
                                                    _np_ptr(ids), _np_ptr(dists)), "dpq_ivf_search_filtered")
        return ids, dists

    def search_probes(self, queries, probes, top_k, id_filter=None):
        """search over the caller's own lists: probes int32 [nq][nprobe], -1 = padding (dpq_ivf_search_probes; with
        `id_filter`, dpq_ivf_search_probes_filtered)."""
        q = self._queries(queries)
        p = self._probes(probes, q.shape[0])
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        if id_filter is None:
            check(self._lib.dpq_ivf_search_probes(self._h, _np_ptr(q), q.shape[0], _np_ptr(p), p.shape[1], top_k, _np_ptr(ids),
                                                  _np_ptr(dists)), "dpq_ivf_search_probes")
        else:
            check(self._lib.dpq_ivf_search_probes_filtered(self._h, IdFilter._handle(id_filter), _np_ptr(q), q.shape[0],
                                                           _np_ptr(p), p.shape[1], top_k, _np_ptr(ids), _np_ptr(dists)),
                  "dpq_ivf_search_probes_filtered")
        return ids, dists

    def search_probes_tables(self, tables, probes, top_k, id_filter=None):
        """search_probes with the caller's distance tables [nq][M][K] standing where the L2 tables of the queries stand
        (dpq_ivf_search_probes_tables); needs no codebook.  Entries: finite >= 0 or +inf."""
        t = self._index._tables(tables)
        p = self._probes(probes, t.shape[0])
        ids = np.empty((t.shape[0], top_k), dtype=np.int32)
        dists = np.empty((t.shape[0], top_k), dtype=np.float32)
        check(self._lib.dpq_ivf_search_probes_tables(self._h, self._filter(id_filter), _np_ptr(t), t.shape[0], _np_ptr(p),
                                                     p.shape[1], top_k, _np_ptr(ids), _np_ptr(dists)),
              "dpq_ivf_search_probes_tables")
        return ids, dists

    def probe_ip(self, queries, nprobe):
        """(lists int32 [nq][nprobe], scores float32 [nq][nprobe]): each query's nprobe centroids of largest exact inner
        product, by (score descending, list number) (dpq_ivf_probe_ip)."""
        q = self._queries(queries)
        lists = np.empty((q.shape[0], nprobe), dtype=np.int32)
        scores = np.empty((q.shape[0], nprobe), dtype=np.float32)
        check(self._lib.dpq_ivf_probe_ip(self._h, _np_ptr(q), q.shape[0], nprobe, _np_ptr(lists), _np_ptr(scores)),
              "dpq_ivf_probe_ip")
        return lists, scores

    def _ip_out(self, nq, top_k):
        return (np.empty((nq, top_k), dtype=np.int32), np.empty((nq, top_k), dtype=np.float32),
                np.empty((nq, top_k), dtype=np.float32), np.empty(nq, dtype=np.float32))

    def search_ip(self, queries, nprobe, top_k, id_filter=None):
        """The top_k codes of the largest approximate inner product among the nprobe lists whose centroids have the
        largest exact inner product with each query (dpq_ivf_search_ip).  Returns (ids, scores descending, gaps, bias) as
        query_batch_ip does; padding is -1 / -inf / +inf."""
        q = self._queries(queries)
        ids, scores, gaps, bias = self._ip_out(q.shape[0], top_k)
        check(self._lib.dpq_ivf_search_ip(self._h, self._filter(id_filter), _np_ptr(q), q.shape[0], nprobe, top_k, _np_ptr(ids),
                                          _np_ptr(scores), _np_ptr(gaps), _np_ptr(bias)), "dpq_ivf_search_ip")
        return ids, scores, gaps, bias

    def search_probes_ip(self, queries, probes, top_k, id_filter=None):
        """search_ip over the caller's own lists (dpq_ivf_search_probes_ip)."""
        q = self._queries(queries)
        p = self._probes(probes, q.shape[0])
        ids, scores, gaps, bias = self._ip_out(q.shape[0], top_k)
        check(self._lib.dpq_ivf_search_probes_ip(self._h, self._filter(id_filter), _np_ptr(q), q.shape[0], _np_ptr(p), p.shape[1],
                                                 top_k, _np_ptr(ids), _np_ptr(scores), _np_ptr(gaps), _np_ptr(bias)),
              "dpq_ivf_search_probes_ip")
        return ids, scores, gaps, bias

    def _radii(self, radius, nq):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))

    def range_search(self, queries, nprobe, radius, id_filter=None):
        """Every code of the nprobe nearest lists within `radius` of each query, d < radius strictly
        (dpq_ivf_range_search).  `radius`: a scalar or one value per query.  Returns what DeltaPQIndex.range_search
        returns: (lims int64 [nq + 1], ids int32, dists float32), each list ascending by (distance, id)."""
        q = self._queries(queries)
        r = self._radii(radius, q.shape[0])
        res = ctypes.c_void_p()
        check(self._lib.dpq_ivf_range_search(self._h, self._filter(id_filter), _np_ptr(q), q.shape[0], nprobe, _np_ptr(r), res),
              "dpq_ivf_range_search")
        return _range_result(self._lib, res)

    def range_search_probes(self, queries, probes, radius, id_filter=None):
        """range_search over the caller's own lists (dpq_ivf_range_search_probes)."""
        q = self._queries(queries)
        p = self._probes(probes, q.shape[0])
        r = self._radii(radius, q.shape[0])
        res = ctypes.c_void_p()
        check(self._lib.dpq_ivf_range_search_probes(self._h, self._filter(id_filter), _np_ptr(q), q.shape[0], _np_ptr(p),
                                                    p.shape[1], _np_ptr(r), res), "dpq_ivf_range_search_probes")
        return _range_result(self._lib, res)

    @staticmethod
    def _torch_out(queries, top_k, out_ids, out_dists):
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous() and queries.dim() in (2, 3)
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        return nq, out_ids, out_dists, ctypes.c_void_p(torch.cuda.current_stream(queries.device).cuda_stream)

    @staticmethod
    def _torch_probes(probes, nq):
        import torch
        assert probes.is_cuda and probes.dtype == torch.int32 and probes.is_contiguous() and probes.dim() == 2
        assert probes.shape[0] == nq
        return ctypes.c_void_p(probes.data_ptr()), probes.shape[1]

    def search_torch(self, queries, nprobe, top_k, out_ids=None, out_dists=None, id_filter=None):
        """search on device tensors, synchronous on torch's current stream (dpq_ivf_search_device[_filtered])."""
        nq, out_ids, out_dists, stream = self._torch_out(queries, top_k, out_ids, out_dists)
        assert queries.dim() == 2
        if id_filter is None:
            check(self._lib.dpq_ivf_search_device(self._h, ctypes.c_void_p(queries.data_ptr()), nq, nprobe, top_k,
                                                  ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_dists.data_ptr()), stream),
                  "dpq_ivf_search_device")
        else:
            check(self._lib.dpq_ivf_search_device_filtered(self._h, IdFilter._handle(id_filter), ctypes.c_void_p(queries.data_ptr()),
                                                           nq, nprobe, top_k, ctypes.c_void_p(out_ids.data_ptr()),
                                                           ctypes.c_void_p(out_dists.data_ptr()), stream),
                  "dpq_ivf_search_device_filtered")
        return out_ids, out_dists

    def search_probes_torch(self, queries, probes, top_k, out_ids=None, out_dists=None, id_filter=None):
        """search_probes on device tensors, synchronous on torch's current stream
        (dpq_ivf_search_probes_device[_filtered])."""
        nq, out_ids, out_dists, stream = self._torch_out(queries, top_k, out_ids, out_dists)
        assert queries.dim() == 2
        pp, nprobe = self._torch_probes(probes, nq)
        if id_filter is None:
            check(self._lib.dpq_ivf_search_probes_device(self._h, ctypes.c_void_p(queries.data_ptr()), nq, pp, nprobe, top_k,
                                                         ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_dists.data_ptr()),
                                                         stream), "dpq_ivf_search_probes_device")
        else:
            check(self._lib.dpq_ivf_search_probes_device_filtered(self._h, IdFilter._handle(id_filter),
                                                                  ctypes.c_void_p(queries.data_ptr()), nq, pp, nprobe, top_k,
                                                                  ctypes.c_void_p(out_ids.data_ptr()),
                                                                  ctypes.c_void_p(out_dists.data_ptr()), stream),
                  "dpq_ivf_search_probes_device_filtered")
        return out_ids, out_dists

    def search_probes_tables_torch(self, tables, probes, top_k, id_filter=None, out_ids=None, out_dists=None):
        """search_probes_tables on device tensors ([nq][M][K] float32, contiguous), synchronous on torch's current
        stream (dpq_ivf_search_probes_device_tables)."""
        nq, out_ids, out_dists, stream = self._torch_out(tables, top_k, out_ids, out_dists)
        assert tables.dim() == 3
        pp, nprobe = self._torch_probes(probes, nq)
        check(self._lib.dpq_ivf_search_probes_device_tables(self._h, self._filter(id_filter), ctypes.c_void_p(tables.data_ptr()),
                                                            nq, pp, nprobe, top_k, ctypes.c_void_p(out_ids.data_ptr()),
                                                            ctypes.c_void_p(out_dists.data_ptr()), stream),
              "dpq_ivf_search_probes_device_tables")
        return out_ids, out_dists

    def search_ip_torch(self, queries, nprobe, top_k, id_filter=None, out_ids=None, out_scores=None, out_gaps=None,
                        out_bias=None):
        """search_ip on device tensors, synchronous on torch's current stream (dpq_ivf_search_device_ip).  Returns
        (ids, scores); gaps and bias are written where out_gaps / out_bias are given."""
        nq, out_ids, out_scores, stream = self._torch_out(queries, top_k, out_ids, out_scores)
        assert queries.dim() == 2
        opt = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        check(self._lib.dpq_ivf_search_device_ip(self._h, self._filter(id_filter), ctypes.c_void_p(queries.data_ptr()), nq, nprobe,
                                                 top_k, ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_scores.data_ptr()),
                                                 opt(out_gaps), opt(out_bias), stream), "dpq_ivf_search_device_ip")
        return out_ids, out_scores

    def search_probes_ip_torch(self, queries, probes, top_k, id_filter=None, out_ids=None, out_scores=None, out_gaps=None,
                               out_bias=None):
        """search_probes_ip on device tensors, synchronous on torch's current stream (dpq_ivf_search_probes_device_ip)."""
        nq, out_ids, out_scores, stream = self._torch_out(queries, top_k, out_ids, out_scores)
        assert queries.dim() == 2
        pp, nprobe = self._torch_probes(probes, nq)
        opt = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        check(self._lib.dpq_ivf_search_probes_device_ip(self._h, self._filter(id_filter), ctypes.c_void_p(queries.data_ptr()), nq,
                                                        pp, nprobe, top_k, ctypes.c_void_p(out_ids.data_ptr()),
                                                        ctypes.c_void_p(out_scores.data_ptr()), opt(out_gaps), opt(out_bias),
                                                        stream), "dpq_ivf_search_probes_device_ip")
        return out_ids, out_scores

    def close(self):
        if self._h is not None:
            self._lib.dpq_ivf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FlatIdFilter:
    """A filter of FlatIndex / FlatIndexU8 / FlatIndexI8 / FlatIndexBits .search_filtered and .range_search (dpq_flat_filter): the set of reported ids
    (row + id_offset) a search may return, compacted once on the index's device into a list of eligible rows.  The bitmap
    convention is IdFilter's; ids at or beyond n_bits are not allowed."""

    pack_mask = staticmethod(IdFilter.pack_mask)
    pack_ids = staticmethod(IdFilter.pack_ids)
    unpack = staticmethod(IdFilter.unpack)

    def __init__(self, flat_index, words, n_bits):
        self._lib = _lib.load()
        self._h = None
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if n_bits < 0 or w.size < (n_bits + 31) // 32:
            raise ValueError("words must hold n_bits >= 0 bits")
        h = ctypes.c_void_p()
        check(self._lib.dpq_flat_filter_create(flat_index._h, _np_ptr(w) if w.size else None, int(n_bits), h),
              "dpq_flat_filter_create")
        self._h = h

    @classmethod
    def from_mask(cls, flat_index, mask):
        """mask[i]: whether reported id i is allowed."""
        return cls(flat_index, *cls.pack_mask(mask))

    @classmethod
    def from_ids(cls, flat_index, ids, n_bits=None):
        return cls(flat_index, *cls.pack_ids(ids, n_bits))

    @staticmethod
    def _handle(f, optional=False):
        if f is None and optional:
            return None
        if not isinstance(f, FlatIdFilter):
            raise TypeError("id_filter must be a FlatIdFilter")
        return f._h

    @property
    def n_allowed(self):
        """Rows of its index the filter allows."""
        n = _lib.c_i64()
        check(self._lib.dpq_flat_filter_count(self._h, n), "dpq_flat_filter_count")
        return n.value

    def close(self):
        if self._h is not None:
            self._lib.dpq_flat_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _range_result(lib, res):
    """A dpq_range_result -> (lims int64 [nq + 1], ids int32, dists float32), copied; the result is freed."""
    try:
        n = _lib.c_i32()
        pl, pi, pd = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.dpq_range_result_get(res, n, pl, pi, pd), "dpq_range_result_get")
        lims = np.ctypeslib.as_array(ctypes.cast(pl, ctypes.POINTER(_lib.c_i64)), (n.value + 1,)).copy()
        total = int(lims[-1])
        ids = np.empty(total, dtype=np.int32)
        dists = np.empty(total, dtype=np.float32)
        if total:
            ctypes.memmove(ids.ctypes.data, pi.value, total * 4)
            ctypes.memmove(dists.ctypes.data, pd.value, total * 4)
        return lims, ids, dists
    finally:
        lib.dpq_range_result_free(res)


class _FlatIndexBase:
    """The methods of every flat index.  A subclass opens the handle (self._lib, self._h, self.n, self.D, self.id_offset),
    says what it takes as queries (_queries for arrays, _check_tensor for tensors) and names its C entry points by the
    suffixes _l2 / _ip: dpq_flat_search + suffix, dpq_flat_rerank + suffix + _device, and so on."""

    _l2, _ip = "", "_ip"

    @property
    def _qcols(self):
        """Elements of one query: D, or the bytes of D bits."""
        return self.D

    def _queries(self, queries):
        q = self._as_queries(queries)
        if q.ndim != 2 or q.shape[1] != self._qcols:
            raise ValueError("queries must be [nq][%d]" % self._qcols)
        return q

    def _search(self, name, queries, top_k, *id_filter):
        """dpq_flat_search*, or, given an id_filter, dpq_flat_search_filtered*."""
        q = self._queries(queries)
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        filt = [FlatIdFilter._handle(f) for f in id_filter]
        check(getattr(self._lib, name)(self._h, *filt, _np_ptr(q), q.shape[0], top_k, _np_ptr(ids), _np_ptr(dists)), name)
        return ids, dists

    def search(self, queries, top_k):
        """Exact top_k over all vectors -> ids int32 [nq][top_k], dists float32 [nq][top_k] by (distance, id)."""
        return self._search("dpq_flat_search" + self._l2, queries, top_k)

    def search_ip(self, queries, top_k):
        """Exact top_k by inner product -> ids int32 [nq][top_k], scores float32 [nq][top_k] by (score descending, id)
        (dpq_flat_search_ip*)."""
        return self._search("dpq_flat_search" + self._ip, queries, top_k)

    def search_filtered(self, queries, top_k, id_filter):
        """Exact top_k over the rows `id_filter` (a FlatIdFilter made on this index) allows; rows are padded with -1 / +inf
        where fewer than top_k rows are allowed (dpq_flat_search_filtered*)."""
        return self._search("dpq_flat_search_filtered" + self._l2, queries, top_k, id_filter)

    def search_filtered_ip(self, queries, top_k, id_filter):
        """search_ip over the rows `id_filter` allows; rows are padded with -1 / -inf (dpq_flat_search_filtered_ip*)."""
        return self._search("dpq_flat_search_filtered" + self._ip, queries, top_k, id_filter)

    def _range_search(self, name, queries, radius, id_filter):
        q = self._queries(queries)
        nq = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        res = ctypes.c_void_p()
        check(getattr(self._lib, name)(self._h, FlatIdFilter._handle(id_filter, optional=True), _np_ptr(q), nq, _np_ptr(r),
                                       res), name)
        return _range_result(self._lib, res)

    def range_search(self, queries, radius, id_filter=None):
        """Every (allowed) row with exact distance d < radius, strictly (dpq_flat_range_search*).  `radius` is a scalar or
        one value per query.  Returns (lims int64 [nq + 1], ids int32, dists float32) as DeltaPQIndex.range_search does;
        query i owns entries lims[i]:lims[i + 1], ascending by (distance, id)."""
        return self._range_search("dpq_flat_range_search" + self._l2, queries, radius, id_filter)

    def range_search_ip(self, queries, threshold, id_filter=None):
        """Every (allowed) row with exact score s > threshold, strictly (dpq_flat_range_search_ip*).  `threshold` is a
        scalar or one value per query.  Returns (lims int64 [nq + 1], ids int32, scores float32); query i owns entries
        lims[i]:lims[i + 1], by (score descending, id)."""
        return self._range_search("dpq_flat_range_search" + self._ip, queries, threshold, id_filter)

    def set_id_map(self, vec_id):
        """DFS position -> row of this handle (DeltaTree.vec_id): rerank candidates are then DFS positions."""
        m = np.ascontiguousarray(vec_id, dtype=np.uint32)
        check(self._lib.dpq_flat_set_id_map(self._h, _np_ptr(m), m.size), "dpq_flat_set_id_map")

    def _rerank(self, name, queries, cand_ids, top_k):
        q = self._queries(queries)
        c = np.ascontiguousarray(cand_ids, dtype=np.int32)
        if c.ndim != 2 or c.shape[0] != q.shape[0]:
            raise ValueError("cand_ids must be [nq][n_cand]")
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        check(getattr(self._lib, name)(self._h, _np_ptr(q), q.shape[0], _np_ptr(c), c.shape[1], top_k, _np_ptr(ids),
                                       _np_ptr(dists)), name)
        return ids, dists

    def rerank(self, queries, cand_ids, top_k):
        """Exact distances of cand_ids[nq][n_cand] only (negative = padding), the best top_k of them."""
        return self._rerank("dpq_flat_rerank" + self._l2, queries, cand_ids, top_k)

    def rerank_ip(self, queries, cand_ids, top_k):
        """Exact inner-product scores of cand_ids[nq][n_cand] only (negative = padding), the best top_k of them by (score
        descending, id); rows are padded with -1 / -inf (dpq_flat_rerank_ip*)."""
        return self._rerank("dpq_flat_rerank" + self._ip, queries, cand_ids, top_k)

    def _rerank_torch(self, name, queries, cand_ids, top_k, out_ids, out_dists):
        import torch
        self._check_tensor(queries)
        assert queries.is_cuda and queries.is_contiguous() and queries.shape[1] == self._qcols
        assert cand_ids.is_cuda and cand_ids.dtype == torch.int32 and cand_ids.is_contiguous()
        assert cand_ids.shape[0] == queries.shape[0]
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        check(getattr(self._lib, name)(self._h, ctypes.c_void_p(queries.data_ptr()), nq,
                                       ctypes.c_void_p(cand_ids.data_ptr()), cand_ids.shape[1], top_k,
                                       ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_dists.data_ptr()),
                                       ctypes.c_void_p(stream)), name)
        return out_ids, out_dists

    def rerank_torch(self, queries, cand_ids, top_k, out_ids=None, out_dists=None):
        """rerank on device tensors, on torch's current stream (dpq_flat_rerank*_device); the results are complete on
        return."""
        return self._rerank_torch("dpq_flat_rerank%s_device" % self._l2, queries, cand_ids, top_k, out_ids, out_dists)

    def rerank_ip_torch(self, queries, cand_ids, top_k, out_ids=None, out_scores=None):
        """rerank_ip on device tensors, on torch's current stream (dpq_flat_rerank_ip*_device); complete on return."""
        return self._rerank_torch("dpq_flat_rerank%s_device" % self._ip, queries, cand_ids, top_k, out_ids, out_scores)

    def close(self):
        if self._h is not None:
            self._lib.dpq_flat_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FlatIndex(_FlatIndexBase):
    """Raw fp32 vectors [n][D] on one GPU (dpq_flat): exact squared L2 distances with the reference's brute-force
    arithmetic -- ground truth over all of them (search), or over a candidate list per query (rerank).  The *_ip methods
    are the same searches by exact inner product: scores instead of distances, best (largest) first."""

    def __init__(self, vectors, device=0, id_offset=0):
        self._lib = _lib.load()
        self._h = None
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2:
            raise ValueError("vectors must be [n][D]")
        self.n, self.D, self.id_offset = int(v.shape[0]), int(v.shape[1]), int(id_offset)
        h = ctypes.c_void_p()
        check(self._lib.dpq_flat_open(_np_ptr(v), self.n, self.D, device, id_offset, ctypes.byref(h)), "dpq_flat_open")
        self._h = h

    @staticmethod
    def _as_queries(queries):
        return np.ascontiguousarray(queries, dtype=np.float32)

    @staticmethod
    def _check_tensor(queries):
        import torch
        assert queries.dtype == torch.float32


HALF_FORMATS = {"f16": 1, "bf16": 2}   # DPQ_HALF_F16, DPQ_HALF_BF16


def _half_format(fmt):
    if fmt not in HALF_FORMATS:
        raise ValueError("fmt must be 'f16' or 'bf16'")
    return HALF_FORMATS[fmt]


def half_from_float(a, fmt):
    """float32 array -> uint16 array of the same shape: the bits of the values narrowed to fp16 ('f16') or bf16 ('bf16'),
    round to nearest, ties to even (dpq_half_from_float; host only)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint16)
    check(_lib.load().dpq_half_from_float(_np_ptr(a), a.size, _half_format(fmt), _np_ptr(out)), "dpq_half_from_float")
    return out


def half_to_float(a, fmt):
    """uint16 bits (or a np.float16 array with fmt 'f16') -> the float32 values they stand for, exactly
    (dpq_half_to_float; host only)."""
    a = np.asarray(a)
    if a.dtype == np.float16 and fmt == "f16":
        a = a.view(np.uint16)
    if a.dtype != np.uint16:
        raise TypeError("half_to_float takes uint16 bits (or float16 with fmt 'f16')")
    a = np.ascontiguousarray(a)
    out = np.empty(a.shape, dtype=np.float32)
    check(_lib.load().dpq_half_to_float(_np_ptr(a), a.size, _half_format(fmt), _np_ptr(out)), "dpq_half_to_float")
    return out


class FlatIndexHalf(FlatIndex):
    """fp16 or bf16 vectors [n][D] on one GPU, at half the device memory of FlatIndex: every method of FlatIndex, with
    fp32 queries, and bit for bit FlatIndex's answers over the rows widened to fp32 (half_to_float).  `vectors` is a
    float32 array (narrowed on the GPU, dpq_flat_open_narrowed), or 16-bit data kept as it is (dpq_flat_open_half): a
    np.float16 array (fmt 'f16'), a np.uint16 array of raw bits, or a CPU torch tensor of dtype float16 / bfloat16
    matching fmt."""

    def __init__(self, vectors, fmt="f16", device=0, id_offset=0):
        self._lib = _lib.load()
        self._h = None
        self.fmt = fmt
        code = _half_format(fmt)
        if not isinstance(vectors, np.ndarray) and hasattr(vectors, "is_cuda"):       # a torch tensor
            import torch
            want = {"f16": torch.float16, "bf16": torch.bfloat16}[fmt]
            if vectors.is_cuda or vectors.dtype != want:
                raise TypeError("a tensor must live on the CPU and have dtype %s for fmt '%s'" % (want, fmt))
            vectors = vectors.contiguous().view(torch.int16).numpy().view(np.uint16)
        v = np.asarray(vectors)
        if v.dtype == np.float16:
            if fmt != "f16":
                raise TypeError("a float16 array needs fmt 'f16'")
            v = v.view(np.uint16)
        if v.dtype == np.uint16:
            name = "dpq_flat_open_half"
        elif v.dtype == np.float32:
            name = "dpq_flat_open_narrowed"
        else:
            raise TypeError("vectors must be float32, float16 or uint16 bits (got %s)" % v.dtype)
        v = np.ascontiguousarray(v)
        if v.ndim != 2:
            raise ValueError("vectors must be [n][D]")
        self.n, self.D, self.id_offset = int(v.shape[0]), int(v.shape[1]), int(id_offset)
        h = ctypes.c_void_p()
        check(getattr(self._lib, name)(_np_ptr(v), self.n, self.D, code, device, id_offset, ctypes.byref(h)), name)
        self._h = h


SQ_BITS = (8, 4)   # DPQ_SQ_8BIT, DPQ_SQ_4BIT


def _sq_bits(bits):
    if bits not in SQ_BITS:
        raise ValueError("bits must be 8 or 4")
    return int(bits)


def _sq_quantiser(lo, step, D):
    """lo, step as contiguous float32 [D]; anything that would need a conversion is refused."""
    out = []
    for name, a in (("lo", lo), ("step", step)):
        a = np.asarray(a)
        if a.dtype != np.float32:
            raise TypeError("%s must be float32 (got %s)" % (name, a.dtype))
        if a.shape != (D,):
            raise ValueError("%s must be [%d]" % (name, D))
        out.append(np.ascontiguousarray(a))
    return out


def _sq_rows(vectors):
    v = np.asarray(vectors)
    if v.dtype != np.float32:
        raise TypeError("vectors must be float32 (got %s)" % v.dtype)
    if v.ndim != 2:
        raise ValueError("vectors must be [n][D]")
    return np.ascontiguousarray(v)


def _sq_codes(codes, D, bits):
    c = np.asarray(codes)
    if c.dtype != np.uint8:
        raise TypeError("codes must be uint8 (got %s)" % c.dtype)
    if c.ndim != 2 or c.shape[1] != (D if bits == 8 else (D + 1) // 2):
        raise ValueError("codes must be [n][D] at 8 bits, [n][(D + 1) / 2] at 4 bits")
    return np.ascontiguousarray(c)


def sq_train(vectors, bits=8, device=0):
    """A scalar quantiser trained on float32 vectors [n][D]: (lo, step), float32 [D] each -- the minimum of every
    dimension and (max - min) / (2^bits - 1) (dpq_sq_train; the reduction runs on the GPU)."""
    v, bits = _sq_rows(vectors), _sq_bits(bits)
    lo, step = np.empty(v.shape[1], dtype=np.float32), np.empty(v.shape[1], dtype=np.float32)
    check(_lib.load().dpq_sq_train(_np_ptr(v), v.shape[0], v.shape[1], bits, device, _np_ptr(lo), _np_ptr(step)), "dpq_sq_train")
    return lo, step


def sq_encode(vectors, lo, step, bits=8, device=0):
    """float32 vectors [n][D] -> uint8 codes [n][D] (8 bits) or [n][(D + 1) / 2] (4 bits: dimension 2j in the low nibble
    of byte j), round to nearest, ties to even, saturating (dpq_sq_encode; on the GPU)."""
    v, bits = _sq_rows(vectors), _sq_bits(bits)
    lo, step = _sq_quantiser(lo, step, v.shape[1])
    out = np.empty((v.shape[0], v.shape[1] if bits == 8 else (v.shape[1] + 1) // 2), dtype=np.uint8)
    check(_lib.load().dpq_sq_encode(_np_ptr(v), v.shape[0], v.shape[1], bits, _np_ptr(lo), _np_ptr(step), device, _np_ptr(out)),
          "dpq_sq_encode")
    return out


def sq_decode(codes, lo, step, bits=8):
    """uint8 codes as sq_encode writes them -> the float32 values [n][D] they stand for, lo + code * step with both
    roundings (dpq_sq_decode; host only)."""
    bits = _sq_bits(bits)
    D = int(np.asarray(lo).shape[0]) if np.asarray(lo).ndim == 1 else -1
    lo, step = _sq_quantiser(lo, step, D)
    c = _sq_codes(codes, D, bits)
    out = np.empty((c.shape[0], D), dtype=np.float32)
    check(_lib.load().dpq_sq_decode(_np_ptr(c), c.shape[0], D, bits, _np_ptr(lo), _np_ptr(step), _np_ptr(out)), "dpq_sq_decode")
    return out


class FlatIndexSQ(FlatIndex):
    """Scalar-quantised vectors [n][D] on one GPU, a byte (bits=8) or a nibble (bits=4) per dimension: every method of
    FlatIndex, with fp32 queries, and bit for bit FlatIndex's answers over sq_decode of the codes.  The constructor takes
    codes the caller already has with their quantiser (dpq_flat_open_sq); from_float quantises float32 rows on the GPU
    (dpq_flat_open_quantised)."""

    def __init__(self, codes, lo, step, bits=8, device=0, id_offset=0):
        self._h = None
        bits = _sq_bits(bits)
        D = int(np.asarray(lo).shape[0]) if np.asarray(lo).ndim == 1 else -1
        lo, step = _sq_quantiser(lo, step, D)
        c = _sq_codes(codes, D, bits)
        self._open("dpq_flat_open_sq", c, c.shape[0], D, bits, lo, step, device, id_offset)

    @classmethod
    def from_float(cls, vectors, bits=8, lo=None, step=None, device=0, id_offset=0):
        """float32 vectors [n][D], quantised on the GPU under (lo, step), or, with neither, under the quantiser trained on
        these very rows."""
        v, bits = _sq_rows(vectors), _sq_bits(bits)
        if (lo is None) != (step is None):
            raise ValueError("lo and step are both given or both left out")
        if lo is not None:
            lo, step = _sq_quantiser(lo, step, v.shape[1])
        self = cls.__new__(cls)
        self._h = None
        self._open("dpq_flat_open_quantised", v, v.shape[0], v.shape[1], bits, lo, step, device, id_offset)
        return self

    def _open(self, name, data, n, D, bits, lo, step, device, id_offset):
        self._lib = _lib.load()
        self.n, self.D, self.bits, self.id_offset = int(n), int(D), bits, int(id_offset)
        h = ctypes.c_void_p()
        check(getattr(self._lib, name)(_np_ptr(data), self.n, self.D, bits, None if lo is None else _np_ptr(lo),
                                       None if step is None else _np_ptr(step), device, id_offset, ctypes.byref(h)), name)
        self._h = h

    def quantiser(self):
        """(lo, step, bits) of the handle (dpq_flat_sq_get)."""
        bits = ctypes.c_int()
        lo, step = np.empty(self.D, dtype=np.float32), np.empty(self.D, dtype=np.float32)
        check(self._lib.dpq_flat_sq_get(self._h, ctypes.byref(bits), _np_ptr(lo), _np_ptr(step)), "dpq_flat_sq_get")
        return lo, step, bits.value


class FlatIndexU8(_FlatIndexBase):
    """Byte vectors [n][D] on one GPU (dpq_flat_open_u8): FlatIndex's answers -- the same ids and the same distance bits as
    on the bytes widened to fp32 -- from the int8 matrix cores, at a quarter of the device memory.  The *_ip methods are
    the same searches by exact inner product of the bytes (dpq_flat_*_ip_u8): FlatIndex's *_ip answers over the widened
    rows.  Takes uint8 arrays and tensors only; anything else is a TypeError rather than a conversion."""

    _dtype, _open, _l2, _ip = np.uint8, "dpq_flat_open_u8", "_u8", "_ip_u8"

    def __init__(self, vectors, device=0, id_offset=0):
        self._h = None
        v = self._bytes(vectors, "vectors")
        if v.ndim != 2:
            raise ValueError("vectors must be [n][D]")
        self._lib = _lib.load()
        self.n, self.D, self.id_offset = int(v.shape[0]), int(v.shape[1]), int(id_offset)
        h = ctypes.c_void_p()
        check(getattr(self._lib, self._open)(_np_ptr(v), self.n, self.D, device, id_offset, ctypes.byref(h)), self._open)
        self._h = h

    @classmethod
    def _bytes(cls, a, what):
        if not isinstance(a, np.ndarray) or a.dtype != cls._dtype:
            raise TypeError("%s must be a %s array (FlatIndex takes fp32)" % (what, np.dtype(cls._dtype).name))
        return np.ascontiguousarray(a)

    def _as_queries(self, queries):
        return self._bytes(queries, "queries")

    def _check_tensor(self, queries):
        import torch
        want = getattr(torch, np.dtype(self._dtype).name)
        if not isinstance(queries, torch.Tensor) or queries.dtype != want:
            raise TypeError("queries must be a %s tensor (FlatIndex takes fp32)" % np.dtype(self._dtype).name)


class FlatIndexI8(FlatIndexU8):
    """Signed byte vectors [n][D] on one GPU (dpq_flat_open_i8): int8 embeddings as they are, searched with int8 queries by
    squared L2 or by inner product (dpq_flat_*_i8, dpq_flat_*_ip_i8) -- every method of FlatIndexU8, and bit for bit
    FlatIndex's answers over the rows widened to fp32.  Takes C-contiguous int8 arrays and int8 tensors only."""

    _dtype, _open, _l2, _ip = np.int8, "dpq_flat_open_i8", "_i8", "_ip_i8"

    @classmethod
    def _bytes(cls, a, what):
        if not isinstance(a, np.ndarray) or a.dtype != np.int8 or not a.flags.c_contiguous:
            raise TypeError("%s must be a C-contiguous int8 array (FlatIndexU8 takes uint8, FlatIndex fp32)" % what)
        return a


def _bits_thresholds(thresholds, D):
    if thresholds is None:
        return None
    t = np.asarray(thresholds)
    if t.dtype != np.float32:
        raise TypeError("thresholds must be float32 (got %s)" % t.dtype)
    if t.shape != (D,):
        raise ValueError("thresholds must be [%d]" % D)
    return np.ascontiguousarray(t)


def bits_from_float(vectors, thresholds=None, device=0):
    """float32 vectors [n][D] -> uint8 [n][(D + 7) // 8] packed bits, bit d = vectors[:, d] > thresholds[d] (> 0 without
    thresholds), dimension d in bit d & 7 of byte d >> 3, spare bits 0 (dpq_bits_from_float; on the GPU)."""
    v = _sq_rows(vectors)
    t = _bits_thresholds(thresholds, v.shape[1])
    out = np.empty((v.shape[0], (v.shape[1] + 7) // 8), dtype=np.uint8)
    check(_lib.load().dpq_bits_from_float(_np_ptr(v), v.shape[0], v.shape[1], None if t is None else _np_ptr(t), device,
                                          _np_ptr(out)), "dpq_bits_from_float")
    return out


class FlatIndexBits(FlatIndexU8):
    """Binary vectors on one GPU, one bit per dimension (dpq_flat_open_bits): `bits` is a uint8 array [n][(D + 7) // 8],
    dimension d in bit d & 7 of byte d >> 3 (np.packbits(..., bitorder="little")); the spare bits of the last byte are
    ignored.  search, search_filtered, range_search, rerank and rerank_torch answer by Hamming distance, reported as a
    float32, in the order and with the padding of the L2 calls (dpq_flat_*_bits); queries are packed the same way.  There
    is no inner product over bits: the *_ip methods raise the library's DpqError.  from_float binarises float32 rows on
    the GPU (dpq_flat_open_binarised).  Takes uint8 arrays and tensors only."""

    _l2, _ip = "_bits", "_ip_u8"

    def __init__(self, bits, D, device=0, id_offset=0):
        self._h = None
        b = self._rows(bits, D, "bits")
        self._lib = _lib.load()
        self.n, self.D, self.id_offset = int(b.shape[0]), int(D), int(id_offset)
        h = ctypes.c_void_p()
        check(self._lib.dpq_flat_open_bits(_np_ptr(b), self.n, self.D, device, id_offset, ctypes.byref(h)), "dpq_flat_open_bits")
        self._h = h

    @classmethod
    def from_float(cls, vectors, thresholds=None, device=0, id_offset=0):
        """float32 vectors [n][D], binarised on the GPU: bit d = vectors[:, d] > thresholds[d] (> 0 without thresholds)."""
        v = _sq_rows(vectors)
        t = _bits_thresholds(thresholds, v.shape[1])
        self = cls.__new__(cls)
        self._h = None
        self._lib = _lib.load()
        self.n, self.D, self.id_offset = int(v.shape[0]), int(v.shape[1]), int(id_offset)
        h = ctypes.c_void_p()
        check(self._lib.dpq_flat_open_binarised(_np_ptr(v), self.n, self.D, None if t is None else _np_ptr(t), device, id_offset,
                                                ctypes.byref(h)), "dpq_flat_open_binarised")
        self._h = h
        return self

    @classmethod
    def _rows(cls, a, D, what):
        a = cls._bytes(a, what)
        if a.ndim != 2 or a.shape[1] != (int(D) + 7) // 8:
            raise ValueError("%s must be [n][(D + 7) // 8] = [n][%d]" % (what, (int(D) + 7) // 8))
        return a

    @classmethod
    def _bytes(cls, a, what):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
            raise TypeError("%s must be a uint8 array of packed bits, eight dimensions to a byte" % what)
        return np.ascontiguousarray(a)

    @property
    def _qcols(self):
        return (self.D + 7) // 8


class RefineLevel:
    """A second PQ level over the residuals of an index's nodes (dpq_refine): M2 more bytes per node, and a PQ
    shortlist is re-ranked by the distance to the two-level reconstruction -- no raw vectors on the GPU.  Made on one
    DeltaPQIndex (after set_codebook) and closed before it."""

    def __init__(self, index, handle):
        self._lib = _lib.load()
        self.index = index
        self._h = handle
        m2, k2, ds2, n = _lib.c_i32(), _lib.c_i32(), _lib.c_i32(), _lib.c_i64()
        check(self._lib.dpq_refine_get(self._h, m2, k2, ds2, n, None, None), "dpq_refine_get")
        self.M2, self.K2, self.Ds2, self.n_local = m2.value, k2.value, ds2.value, n.value
        inf = index.info()
        self.D1 = inf["M"] * inf["Ds"]

    @classmethod
    def build(cls, index, vectors, vec_id=None, M2=0, K2=0, train_n=0, max_iters=0, seed=0, start="rows", restarts=0):
        """Trains and encodes a level from raw vectors [n_rows][D] (dpq_refine_build).  The row of the handle's local
        node l is vectors[vec_id[l]] (DeltaTree.vec_id's slice for the handle), or vectors[l] without a map."""
        if start not in _TRAIN_STARTS:
            raise ValueError('start must be "rows" or "kmeans++"')
        lib = _lib.load()
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2:
            raise ValueError("vectors must be [n_rows][D]")
        vid = None if vec_id is None else np.ascontiguousarray(vec_id, dtype=np.uint32).ravel()
        if vid is not None and vid.size != index.info()["node_hi"] - index.info()["node_lo"]:
            raise ValueError("vec_id must hold one entry per node of the handle")
        opts = _lib.RefineOpts(M2=M2, K2=K2, train_n=train_n, max_iters=max_iters, init=_TRAIN_STARTS[start],
                               restarts=restarts, seed=seed)
        h = ctypes.c_void_p()
        check(lib.dpq_refine_build(index._h, _np_ptr(v), v.shape[0], v.shape[1], None if vid is None else _np_ptr(vid), opts,
                                   ctypes.byref(h)), "dpq_refine_build")
        return cls(index, h)

    @classmethod
    def from_arrays(cls, index, codewords2, codes2):
        """Uploads a ready-made level (dpq_refine_create): codewords2 float32 [M2][K2][Ds2], codes2 uint8 [n_local][M2]."""
        lib = _lib.load()
        cw = np.ascontiguousarray(codewords2, dtype=np.float32)
        c = np.ascontiguousarray(codes2, dtype=np.uint8)
        if cw.ndim != 3 or c.ndim != 2 or c.shape[1] != cw.shape[0]:
            raise ValueError("codewords2 must be [M2][K2][Ds2] and codes2 [n_local][M2]")
        h = ctypes.c_void_p()
        check(lib.dpq_refine_create(index._h, _np_ptr(cw), cw.shape[0], cw.shape[1], cw.shape[2], _np_ptr(c), c.shape[0],
                                    ctypes.byref(h)), "dpq_refine_create")
        return cls(index, h)

    def arrays(self):
        """(codewords2 float32 [M2][K2][Ds2], codes2 uint8 [n_local][M2]) read back (dpq_refine_get)."""
        cw = np.empty((self.M2, self.K2, self.Ds2), dtype=np.float32)
        c = np.empty((self.n_local, self.M2), dtype=np.uint8)
        check(self._lib.dpq_refine_get(self._h, None, None, None, None, _np_ptr(cw), _np_ptr(c)), "dpq_refine_get")
        return cw, c

    @staticmethod
    def residuals(index, ids, vectors):
        """Row i: vectors[i] (zero padded to M * Ds) minus the level-1 reconstruction of the node ids[i] names
        (dpq_residuals), float32 [n][M * Ds]; a negative id gives NaNs."""
        lib = _lib.load()
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[0] != i.size:
            raise ValueError("vectors must be [len(ids)][D]")
        inf = index.info()
        out = np.empty((i.size, inf["M"] * inf["Ds"]), dtype=np.float32)
        check(lib.dpq_residuals(index._h, _np_ptr(i), i.size, _np_ptr(v), v.shape[1], _np_ptr(out)), "dpq_residuals")
        return out

    def reconstruct(self, ids):
        """The two-level reconstruction of reported ids (dpq_refine_reconstruct), float32 [n][M * Ds]; a negative id gives
        a row of NaNs."""
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        out = np.empty((i.size, self.D1), dtype=np.float32)
        check(self._lib.dpq_refine_reconstruct(self._h, _np_ptr(i), i.size, _np_ptr(out)), "dpq_refine_reconstruct")
        return out

    def _queries(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.D1:
            raise ValueError("queries must be [nq][%d]" % self.D1)
        return q

    def rerank(self, queries, cand_ids, top_k):
        """Refined distances of cand_ids[nq][n_cand] only (negative = padding), the best top_k of them
        (dpq_refine_rerank)."""
        q = self._queries(queries)
        c = np.ascontiguousarray(cand_ids, dtype=np.int32)
        if c.ndim != 2 or c.shape[0] != q.shape[0]:
            raise ValueError("cand_ids must be [nq][n_cand]")
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        check(self._lib.dpq_refine_rerank(self._h, _np_ptr(q), q.shape[0], _np_ptr(c), c.shape[1], top_k, _np_ptr(ids),
                                          _np_ptr(dists)), "dpq_refine_rerank")
        return ids, dists

    def rerank_torch(self, queries, cand_ids, top_k, out_ids=None, out_dists=None):
        """rerank on device tensors, on torch's current stream (dpq_refine_rerank_device); the results are complete on
        return."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous() and queries.shape[1] == self.D1
        assert cand_ids.is_cuda and cand_ids.dtype == torch.int32 and cand_ids.is_contiguous()
        assert cand_ids.shape[0] == queries.shape[0]
        nq = queries.shape[0]
        if out_ids is None:
            out_ids = torch.empty((nq, top_k), dtype=torch.int32, device=queries.device)
        if out_dists is None:
            out_dists = torch.empty((nq, top_k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        check(self._lib.dpq_refine_rerank_device(self._h, ctypes.c_void_p(queries.data_ptr()), nq,
                                                 ctypes.c_void_p(cand_ids.data_ptr()), cand_ids.shape[1], top_k,
                                                 ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_dists.data_ptr()),
                                                 ctypes.c_void_p(stream)), "dpq_refine_rerank_device")
        return out_ids, out_dists

    def query_batch_refined(self, queries, n_cand, top_k, id_filter=None):
        """The PQ top-n_cand of the index (among those `id_filter` allows, when given) refined to top_k, without a host
        round trip in between (dpq_query_batch_refined)."""
        q = self._queries(queries)
        ids = np.empty((q.shape[0], top_k), dtype=np.int32)
        dists = np.empty((q.shape[0], top_k), dtype=np.float32)
        f = None if id_filter is None else IdFilter._handle(id_filter)
        check(self._lib.dpq_query_batch_refined(self.index._h, self._h, f, _np_ptr(q), q.shape[0], n_cand, top_k,
                                                _np_ptr(ids), _np_ptr(dists)), "dpq_query_batch_refined")
        return ids, dists

    def close(self):
        if self._h is not None:
            self._lib.dpq_refine_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_vecs_range(path, first, count, ext="fvecs"):
    """Vectors [first, first + count) of an .fvecs/.bvecs file -> float32 [count][D]."""
    lib = _lib.load()
    D = _lib.c_i32()
    check(lib.dpq_read_vecs_range(path.encode(), int(ext == "bvecs"), first, count, D, None), "dpq_read_vecs_range")
    out = np.empty((count, D.value), dtype=np.float32)
    check(lib.dpq_read_vecs_range(path.encode(), int(ext == "bvecs"), first, count, D, _np_ptr(out)), "dpq_read_vecs_range")
    return out


def read_bvecs_range(path, first, count):
    """Vectors [first, first + count) of a .bvecs file -> uint8 [count][D], the bytes as they are."""
    lib = _lib.load()
    D = _lib.c_i32()
    check(lib.dpq_read_bvecs_range(path.encode(), first, count, D, None), "dpq_read_bvecs_range")
    out = np.empty((count, D.value), dtype=np.uint8)
    check(lib.dpq_read_bvecs_range(path.encode(), first, count, D, _np_ptr(out)), "dpq_read_bvecs_range")
    return out


def write_groundtruth(path, ids, dists):
    """The reference's ground-truth text file (pqbase.cpp:294-312), distances with nine digits (bit-exact on read)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    assert ids.ndim == 2 and ids.shape == dists.shape
    check(_lib.load().dpq_write_groundtruth(path.encode(), _np_ptr(ids), _np_ptr(dists), ids.shape[0], ids.shape[1]),
          "dpq_write_groundtruth")


def read_groundtruth(path):
    """-> ids int32 [nq][top_k], dists float32 [nq][top_k] (pqbase.cpp:313-332)."""
    lib = _lib.load()
    nq, k = _lib.c_i32(), _lib.c_i32()
    check(lib.dpq_read_groundtruth(path.encode(), nq, k, None, None), "dpq_read_groundtruth")
    ids = np.empty((nq.value, k.value), dtype=np.int32)
    dists = np.empty((nq.value, k.value), dtype=np.float32)
    check(lib.dpq_read_groundtruth(path.encode(), nq, k, _np_ptr(ids), _np_ptr(dists)), "dpq_read_groundtruth")
    return ids, dists


def recall(found, truth, k=None, R=None):
    """Mean over queries of |found[q][:R] & truth[q][:k]| / k, negative ids ignored (dpq_recall).  R = k (the default:
    k = truth's width, R = k) is the reference's measure (main.cpp:783-796); k = 1 gives 1-recall@R."""
    found = np.ascontiguousarray(found, dtype=np.int32)
    truth = np.ascontiguousarray(truth, dtype=np.int32)
    assert found.ndim == 2 and truth.ndim == 2 and found.shape[0] == truth.shape[0]
    k = truth.shape[1] if k is None else k
    R = min(k, found.shape[1]) if R is None else R
    out = ctypes.c_double()
    check(_lib.load().dpq_recall(_np_ptr(found), found.shape[1], R, _np_ptr(truth), truth.shape[1], k, found.shape[0], out),
          "dpq_recall")
    return out.value


def range_recall(found, truth):
    """(recall, precision) of a range answer against the truth, both (lims, ids[, dists]) over the same queries and in the
    same id space, summed over the queries (dpq_range_recall); a zero denominator gives 1.0."""
    fl = np.ascontiguousarray(found[0], dtype=np.int64)
    fi = np.ascontiguousarray(found[1], dtype=np.int32)
    tl = np.ascontiguousarray(truth[0], dtype=np.int64)
    ti = np.ascontiguousarray(truth[1], dtype=np.int32)
    if fl.ndim != 1 or fl.shape != tl.shape or fl.size < 1 or fi.size < fl[-1] or ti.size < tl[-1]:
        raise ValueError("found and truth must be (lims [nq + 1], ids [lims[-1]]) over the same queries")
    rec, prec = ctypes.c_double(), ctypes.c_double()
    check(_lib.load().dpq_range_recall(fl.size - 1, _np_ptr(fl), _np_ptr(fi) if fi.size else None, _np_ptr(tl),
                                       _np_ptr(ti) if ti.size else None, rec, prec), "dpq_range_recall")
    return rec.value, prec.value


def bitmap_to_dfs(words, n_bits, vec_id):
    """A bitmap over original vector ids -> (words, n_bits) of the bitmap IdFilter takes for the DTC index whose DFS
    position p holds vector vec_id[p] (dpq_bitmap_to_dfs; the even-N rule applied)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    v = np.ascontiguousarray(vec_id, dtype=np.uint32)
    if n_bits < 0 or w.size < (n_bits + 31) // 32:
        raise ValueError("words must hold n_bits >= 0 bits")
    out = np.zeros((v.size + 1 + 31) // 32, dtype=np.uint32)
    check(_lib.load().dpq_bitmap_to_dfs(_np_ptr(w) if w.size else None, int(n_bits), _np_ptr(v), v.size, _np_ptr(out)),
          "dpq_bitmap_to_dfs")
    return out, v.size + 1


def write_bitmap(path, words, n_bits):
    """A bitmap file: int64 n_bits, then (n_bits + 31) // 32 little-endian uint32 words (dpq_write_bitmap)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if n_bits < 0 or w.size < (n_bits + 31) // 32:
        raise ValueError("words must hold n_bits >= 0 bits")
    check(_lib.load().dpq_write_bitmap(path.encode(), _np_ptr(w) if w.size else None, int(n_bits)), "dpq_write_bitmap")


def read_bitmap(path):
    """-> (words uint32 [(n_bits + 31) // 32], n_bits) (dpq_read_bitmap)."""
    lib = _lib.load()
    n = _lib.c_i64()
    check(lib.dpq_read_bitmap(path.encode(), n, None), "dpq_read_bitmap")
    words = np.zeros((n.value + 31) // 32, dtype=np.uint32)
    check(lib.dpq_read_bitmap(path.encode(), n, _np_ptr(words) if words.size else None), "dpq_read_bitmap")
    return words, n.value


def pin_host(arr):
    """Page-lock a numpy array's memory (hipHostRegister through the library): host-to-host batches then overlap their copies."""
    check(_lib.load().dpq_pin_host(_np_ptr(arr), arr.nbytes), "dpq_pin_host")
    return arr


def unpin_host(arr):
    check(_lib.load().dpq_unpin_host(_np_ptr(arr)), "dpq_unpin_host")


def merge_topk_host(ids, dists):
    """ids/dists [n_lists][nq][k] -> merged [nq][k] by (distance, id)."""
    lib = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    n_lists, nq, k = ids.shape
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k), dtype=np.float32)
    check(lib.dpq_merge_topk_host(_np_ptr(ids), _np_ptr(dists), n_lists, nq, k, _np_ptr(oi), _np_ptr(od)),
          "dpq_merge_topk_host")
    return oi, od


def merge_topk_ip_host(ids, scores):
    """ids/scores [n_lists][nq][k] -> merged [nq][k] by (score descending, id); padding is -1 / -inf
    (dpq_merge_topk_ip_host; host only, no device)."""
    lib = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n_lists, nq, k = ids.shape
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k), dtype=np.float32)
    check(lib.dpq_merge_topk_ip_host(_np_ptr(ids), _np_ptr(scores), n_lists, nq, k, _np_ptr(oi), _np_ptr(od)),
          "dpq_merge_topk_ip_host")
    return oi, od


def ip_scores(bias, gaps, ids):
    """float32 [nq][k] inner-product scores of (merged) gaps: (float)((double)bias[q] - (double)gap), -inf for a padding
    row (dpq_ip_scores; host only, no device)."""
    lib = _lib.load()
    g = np.ascontiguousarray(gaps, dtype=np.float32)
    i = np.ascontiguousarray(ids, dtype=np.int32)
    b = np.ascontiguousarray(bias, dtype=np.float32).ravel()
    assert g.ndim == 2 and i.shape == g.shape and b.shape == (g.shape[0],)
    out = np.empty(g.shape, dtype=np.float32)
    check(lib.dpq_ip_scores(_np_ptr(b), _np_ptr(g), _np_ptr(i), g.shape[0], g.shape[1], _np_ptr(out)), "dpq_ip_scores")
    return out


def _merge_out(out, nq, k, device):
    """The [nq][k] int32 / float32 result tensors of a device merge: fresh ones, or the caller's `out` pair."""
    import torch
    if out is None:
        return (torch.empty((nq, k), dtype=torch.int32, device=device),
                torch.empty((nq, k), dtype=torch.float32, device=device))
    oi, od = out
    assert oi.shape == (nq, k) and od.shape == (nq, k) and oi.dtype == torch.int32 and od.dtype == torch.float32
    assert oi.device == device and od.device == device and oi.is_contiguous() and od.is_contiguous()
    return oi, od


def merge_topk_torch(ids, dists, out=None):
    """Device merge after an all-gather: ids/dists [n_lists][nq][k] cuda tensors.  Every list ascending by (distance
    bits, id) with its padding rows (id < 0) last; repeated keys are kept (include/deltapq_amd.h).  `out`: an
    (ids, dists) pair of [nq][k] tensors to write into."""
    import torch
    lib = _lib.load()
    assert ids.is_cuda and ids.is_contiguous() and dists.is_contiguous()
    n_lists, nq, k = ids.shape
    oi, od = _merge_out(out, nq, k, ids.device)
    if nq == 0:
        return oi, od       # an empty tensor has no address to pass
    stream = torch.cuda.current_stream(ids.device).cuda_stream
    check(lib.dpq_merge_topk_device(ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(dists.data_ptr()), n_lists, nq,
                                    k, ctypes.c_void_p(oi.data_ptr()), ctypes.c_void_p(od.data_ptr()),
                                    ids.device.index or 0, ctypes.c_void_p(stream)), "dpq_merge_topk_device")
    return oi, od


def merge_topk_packed_torch(gathered, k, out=None):
    """Device merge straight from the all-gathered tensor [n_lists][nq][2k] int32 (ids | distance bits); the contract
    and `out` of merge_topk_torch."""
    import torch
    lib = _lib.load()
    assert gathered.is_cuda and gathered.is_contiguous() and gathered.dtype == torch.int32 and gathered.shape[2] == 2 * k
    n_lists, nq = gathered.shape[0], gathered.shape[1]
    oi, od = _merge_out(out, nq, k, gathered.device)
    if nq == 0:
        return oi, od
    stream = torch.cuda.current_stream(gathered.device).cuda_stream
    check(lib.dpq_merge_topk_device_packed(ctypes.c_void_p(gathered.data_ptr()), n_lists, nq, k, ctypes.c_void_p(oi.data_ptr()),
                                           ctypes.c_void_p(od.data_ptr()), gathered.device.index or 0, ctypes.c_void_p(stream)),
          "dpq_merge_topk_device_packed")
    return oi, od


# ---------------------------------------------------------------------------
# Reference-named conveniences (one call per query, like main:328-339).
# ---------------------------------------------------------------------------

def query_processing_scan_compressed_codes_opt_in_memory(codes, n_bytes, query, top_k, M, K, m_Ds, num_codes,
                                                         m_codewords, device=0):
    """Signature of deltapq_create_approx_tree.h:3731-3736 (decoder argument dropped).
    Returns results as a list of (id, dist) ascending, like `results` there."""
    payload = np.asarray(codes, dtype=np.uint8)[:n_bytes]
    cb = np.asarray(m_codewords, dtype=np.float32).reshape(M, K, m_Ds)
    with DeltaPQIndex.open_memory(payload, num_codes, M, K, device=device) as idx:
        idx.set_codebook(cb)
        ids, dists = idx.query_batch(np.asarray(query, dtype=np.float32)[None, :], top_k)
    return list(zip(ids[0].tolist(), dists[0].tolist()))


def query_processing_scan_compressed_codes_opt_o_direct(dataset_path, query, top_k, M, K, m_Ds, num_codes,
                                                        m_codewords, device=0):
    """Signature of deltapq_create_approx_tree.h:2805-2810 (decoder argument dropped)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    check(lib.dpq_dtc_file_name(dataset_path.encode(), M, K, num_codes, buf, 4096), "dpq_dtc_file_name")
    cb = np.asarray(m_codewords, dtype=np.float32).reshape(M, K, m_Ds)
    with DeltaPQIndex.open_file(buf.value.decode(), M, K, device=device) as idx:
        idx.set_codebook(cb)
        ids, dists = idx.query_batch(np.asarray(query, dtype=np.float32)[None, :], top_k)
    return list(zip(ids[0].tolist(), dists[0].tolist()))
