"""IVF search over an index of residual codes (include/deltapq_amd.h "IVF search by residual").  The reference is the numpy
restatement of tests/_ivf_residual_restatement.py: r = q - c_l in fp32, the table by the table build's rule, then the fp64
sum rounded once (a DTC handle) or M fp32 additions (a plain handle).  The GPU meets it bit for bit, for every group size
P of the scan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _ivf_restatement as R
import _numeric_edges as ne
from _ivf_residual_restatement import distances, same, search, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_ivf_residuals", "dpq_ivf_residuals_device", "dpq_ivf_search_residual", "dpq_ivf_search_residual_device",
           "dpq_ivf_search_probes_residual", "dpq_ivf_search_probes_residual_device")
F32, F64 = np.float32, np.float64


LENGTHS = (0, 1, 255, 256, 257, 600)  # lists 0 .. 5; list 6 takes the rest
NLIST, NPROBE, NQ = 7, 5, 5
PROBES = np.array([[(q + j) % NLIST for j in range(NPROBE)] for q in range(NQ)], dtype=np.int32)
_cases = {}


def entries(c, labels, nlist, codes, lo=0):
    """What the restatement reads of the lists: offsets, reported ids, and the codes of the entries."""
    n = len(labels)
    c["offsets"], c["ids"] = R.lists_from_labels(labels, nlist, node_lo=lo, n_total=lo + n, even_rule=not c["plain"])
    pos = c["ids"].astype(np.int64) - lo
    pos[pos == n] = n - 1                                                          # the even-N renaming undone
    c["entry_codes"] = codes[pos]


def make_case(M, Ds, K, plain, n=2000, lo=0, labels=None, codes=None, seed=0):
    """One index with its lists, built once per key and left unchanged: payload or plain codes, float codebook, centroids,
    queries."""
    key = (M, Ds, K, plain, n, lo, seed) if labels is None else None
    if key in _cases:
        return _cases[key]
    from deltapq_amd import synth
    rng = np.random.default_rng(100 * M + Ds + seed)
    c = dict(M=M, Ds=Ds, K=K, plain=plain, n=n, lo=lo)
    if plain:
        drawn = rng.integers(0, K, size=(n, M), dtype=np.uint8)                    # (drawn either way: the same cb, cents, qs)
        c["codes"] = drawn if codes is None else codes
    else:
        tree = ne.plain_tree(n, M, K, 7 + seed)
        c["payload"], c["codes"] = synth.encode_dtc(tree)[0], synth.decode_tree_codes(tree)
    if labels is None:
        labels = np.full(n, NLIST - 1, dtype=np.int32)
        labels[rng.permutation(n)[:sum(LENGTHS)]] = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    c["labels"] = labels
    c["cb"] = rng.standard_normal((M, K, Ds)).astype(F32)
    c["cents"] = rng.standard_normal((NLIST, M * Ds)).astype(F32)
    c["qs"] = rng.standard_normal((NQ, M * Ds)).astype(F32)
    entries(c, labels, NLIST, c["codes"], lo)
    if key is not None:
        _cases[key] = c
    return c


def open_case(api, c, centroids=True):
    if c["plain"]:
        idx = api.DeltaPQIndex.open_plain(c["codes"], K=c["K"])
    else:
        opts = dict(global_offset=c["lo"], global_n_codes=c["lo"] + c["n"]) if c["lo"] else {}
        idx = api.DeltaPQIndex.open_memory(c["payload"], c["n"], c["M"], c["K"], **opts)
    idx.set_codebook(c["cb"])
    return idx, api.IVF.from_labels(idx, c["labels"], NLIST, centroids=c["cents"] if centroids else None)


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def with_group(monkeypatch, P):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_IVF_RESIDUAL_GROUP", str(P))


def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared"
        assert name in exported and name in bound and hasattr(lib, name), name


def test_argument_errors_need_no_device(lib):
    """Refused before the structure is looked at (the handle below is never dereferenced) and before a device is asked
    for.  (The state errors -- no centroids, on the probes form too -- need a real structure: test_probe_rows.)"""
    buf, ib = np.zeros(64, dtype=F32), np.zeros(64, dtype=np.int32)
    p, ip, h = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ib.ctypes.data), ctypes.c_void_p(0x1000)
    for fn, with_probes, tail in ((lib.dpq_ivf_search_residual, False, ()), (lib.dpq_ivf_search_residual_device, False, (None,)),
                                  (lib.dpq_ivf_search_probes_residual, True, ()),
                                  (lib.dpq_ivf_search_probes_residual_device, True, (None,))):
        def call(v=h, q=p, nq=1, pr=ip, nprobe=2, k=2, oi=ip, od=p):
            return fn(v, None, q, nq, *((pr, nprobe) if with_probes else (nprobe,)), k, oi, od, *tail)
        bad = [call(v=None), call(q=None), call(oi=None), call(od=None), call(nq=-1), call(k=0), call(k=2049), call(nprobe=0),
               call(nprobe=1025)] + ([call(pr=None)] if with_probes else [])
        assert bad == [ERR_ARG] * len(bad), fn.__name__
    for fn, mid, tail in ((lib.dpq_ivf_residuals, (0,), ()), (lib.dpq_ivf_residuals_device, (), (None,))):
        def call(c=p, nlist=2, D=4, v=p, n=3, l=ip, o=p):
            return fn(c, nlist, D, v, n, l, *mid, o, *tail)
        bad = [call(c=None), call(v=None), call(l=None), call(o=None), call(nlist=0), call(nlist=65537), call(D=0), call(D=2049),
               call(n=-1), call(n=1 << 31)]
        assert bad == [ERR_ARG] * len(bad), fn.__name__
    ib[1] = 2                                                                      # a label that names no list: the host form
    assert lib.dpq_ivf_residuals(p, 2, 4, p, 3, ip, 0, p) == ERR_ARG and b"labels[1]" in lib.dpq_last_error()


def test_the_restatement_against_float64():
    """On finite inputs the restated distance agrees with the float64 ||q - (c_l + x^)||^2 = sum_m sum_d ((q - c) - cb)^2
    within a relative bound, u = 2^-24.  Per dimension: r = fl(q - c) carries |q - c| u, diff = fl(cb - r) another
    |cb - r| u, so |diff - exact| <= (|q| + |c| + |cb| + |r|) u =: e and the square errs by 2 |diff| e + e^2 (the fp64
    square adds 2^-53, ignored against u).  Each of the Ds `float += double` steps rounds a partial sum <= T once:
    Ds u T.  The M terms: the fp64 sum rounds once at the end (u S); the fp32 sum once per addition (M u S).  Hence
    |got - exact| <= sum_{m,d} (2 |diff| e + e^2) + (Ds + M) u S, with S the exact sum; the test asserts that bound with
    the factor (1 + 2^-10) that pays for taking |diff| and S from the exact values."""
    u = 2.0 ** -24
    for (M, Ds, K), plain in [((8, 4, 256), False), ((8, 3, 200), True), ((16, 2, 256), False)]:
        rng = np.random.default_rng(M + Ds)
        cb = rng.standard_normal((M, K, Ds)).astype(F32)
        q, c = rng.standard_normal(M * Ds).astype(F32), rng.standard_normal(M * Ds).astype(F32)
        codes = rng.integers(0, K, size=(500, M), dtype=np.uint8)
        got = distances(table(cb, (q - c).astype(F32)), codes, plain).astype(F64)
        word = cb[np.arange(M), codes].astype(F64)                                 # [n][M][Ds]
        exact_diff = word - (q.astype(F64) - c.astype(F64)).reshape(M, Ds)
        exact = (exact_diff ** 2).sum(axis=(1, 2))
        e = (np.abs(q) + np.abs(c) + np.abs(q - c)).astype(F64).reshape(M, Ds) * u + np.abs(word) * u
        bound = ((2 * np.abs(exact_diff) * e + e * e).sum(axis=(1, 2)) + (Ds + M) * u * exact) * (1 + 2.0 ** -10)
        assert np.all(np.abs(got - exact) <= bound), (M, Ds, K, plain, np.max(np.abs(got - exact) / bound))


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
@pytest.mark.parametrize("shape", [(8, 4, 256), (8, 3, 200), (16, 2, 256)])
def test_definition(gpu, monkeypatch, shape, plain):
    """Lists of 0, 1, 255, 256, 257 entries and longer; nprobe = 5, so the last group is ragged at P = 2 and P = 4; Ds = 3
    takes the scalar path, K = 200 the +inf tail; n = 2000 is even, so the DTC handle renames its last node."""
    c = make_case(*shape, plain)
    assert np.diff(c["offsets"]).tolist()[:6] == list(LENGTHS)
    idx, ivf = open_case(gpu, c)
    with idx, ivf:
        for k in (1, 100):
            want = search(c, c["qs"], PROBES, k)
            for P in (1, 2, 4):
                with_group(monkeypatch, P)
                assert same(ivf.search_probes_residual(c["qs"], PROBES, k), want), (shape, plain, k, P)


@pytest.mark.gpu
def test_threshold_refresh_across_the_lists_of_a_group(gpu, monkeypatch):
    """List 0 holds 1500 entries (> 2 * 256 + 256) ordered so that its best keys come last -- every refresh lowers the
    threshold -- and the short lists 1 and 2 behind it in the same group lie much farther from their centroids: a count, a
    parity or a threshold carried over from list 0 would drop their entries."""
    M, Ds, K, n = 8, 4, 256, 2000
    labels = np.repeat(np.array([0, 1, 2, 3], dtype=np.int32), [1500, 50, 300, 150])
    c = make_case(M, Ds, K, True, n=n, labels=labels, seed=1)
    order = np.argsort(-distances(table(c["cb"], (c["qs"][0] - c["cents"][0]).astype(F32)), c["codes"][:1500], True), kind="stable")
    c = make_case(M, Ds, K, True, n=n, labels=labels, codes=np.concatenate([c["codes"][:1500][order], c["codes"][1500:]]), seed=1)
    c["cents"][1:3] += 40.0
    probes = np.array([[0, 1, 2, -1], [2, 0, 1, 3]], dtype=np.int32)
    want = search(c, c["qs"][:2], probes, 100)
    assert want[0][0][0] == 1499 and np.all(want[0][0][:100] >= 1400)              # query 0: the best of list 0 are its last
    one = search(c, c["qs"][:1], [[1]], 100)
    assert one[1][0][0] > want[1][0][99]                                           # list 1 starts above list 0's last threshold
    idx, ivf = open_case(gpu, c)
    with idx, ivf:
        with_group(monkeypatch, 4)
        assert same(ivf.search_probes_residual(c["qs"][:2], probes, 100), want)
        assert same(ivf.search_probes_residual(c["qs"][:1], [[1]], 100), one)


@pytest.mark.gpu
def test_probe_rows(gpu, monkeypatch):
    """Padding and repeats inside a group; search_residual is probe followed by search_probes_residual; an entry >= nlist;
    every residual form needs centroids."""
    c = make_case(8, 4, 256, False)
    probes = np.array([[-1, 3, 3, 6, -1, 2, 3], [5, 5, 5, 5, 4, -1, -1], [-1] * 7, [0, 0, 1, 1, 0, -1, 6], [6, 5, 4, 3, 2, 1, 0]],
                      dtype=np.int32)                                              # (nprobe <= nlist = 7)
    idx, ivf = open_case(gpu, c)
    with idx, ivf:
        for P in (1, 2, 4):
            with_group(monkeypatch, P)
            assert same(ivf.search_probes_residual(c["qs"], probes, 100), search(c, c["qs"], probes, 100)), P
        lists, _ = ivf.probe(c["qs"], 3)
        assert same(ivf.search_residual(c["qs"], 3, 10), ivf.search_probes_residual(c["qs"], lists, 10))
        assert same(ivf.search_residual(c["qs"], 3, 10), search(c, c["qs"], lists, 10))
        probes[1, 2] = NLIST
        with pytest.raises(gpu.DpqError) as e:
            ivf.search_probes_residual(c["qs"], probes, 10)
        assert e.value.status == ERR_ARG
    idx, ivf = open_case(gpu, c, centroids=False)
    with idx, ivf:
        for call in (lambda: ivf.search_probes_residual(c["qs"], PROBES, 10), lambda: ivf.search_residual(c["qs"], 3, 10)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == ERR_STATE and "centroids" in str(e.value)
        ivf.search_probes(c["qs"], PROBES, 10)                                     # (the non-residual probes form needs none)


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
def test_against_the_shipped_search(gpu, plain):
    """Any centroids: the answer restricted to list l is search_probes of the query q - c_l over the probe row {l}.  Zero
    centroids: the residual search is search_probes, bit for bit."""
    c = make_case(8, 4, 256, plain)
    idx, ivf = open_case(gpu, c)
    with idx, ivf:
        for q in c["qs"][:3]:
            for l in range(NLIST):
                got = ivf.search_probes_residual(q, [[l]], 100)
                assert same(got, ivf.search_probes((q - c["cents"][l]).astype(F32), [[l]], 100)), (plain, l)
        ivf.set_centroids(np.zeros_like(c["cents"]))
        assert same(ivf.search_probes_residual(c["qs"], PROBES, 100), ivf.search_probes(c["qs"], PROBES, 100))


@pytest.mark.gpu
@pytest.mark.parametrize("lo", [0, 1000002], ids=["even_n", "part"])
def test_filter(gpu, monkeypatch, lo):
    """About 10 % allowed, and nothing allowed in list 5, on a DTC handle whose last node is renamed (n and lo + n even)
    and on a part with a non-zero id_base."""
    c = make_case(8, 4, 256, False, lo=lo)
    n_ids = lo + c["n"] + 1
    assert c["ids"].max() == n_ids - 1                                             # the renamed node is in a list
    allowed = np.zeros(n_ids, dtype=bool)
    allowed[lo:] = np.random.default_rng(3).random(c["n"] + 1) < 0.1
    allowed[n_ids - 1] = True
    allowed[c["ids"][c["offsets"][5]:c["offsets"][6]]] = False
    idx, ivf = open_case(gpu, c)
    with idx, ivf, gpu.IdFilter.from_mask(idx, allowed) as f:
        for P in (1, 4):
            with_group(monkeypatch, P)
            for k in (1, 100):
                got = ivf.search_probes_residual(c["qs"], PROBES, k, id_filter=f)
                assert same(got, search(c, c["qs"], PROBES, k, allowed)), (lo, P, k)
        only5 = ivf.search_probes_residual(c["qs"], [[5]] * NQ, 10, id_filter=f)
        assert np.all(only5[0] == -1) and np.all(np.isposinf(only5[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 8])
def test_ivf_residuals(gpu, D):
    import torch
    rng = np.random.default_rng(D)
    n, nlist = 1000, 5                                                             # n is no multiple of 256
    v, cents = rng.standard_normal((n, D)).astype(F32), rng.standard_normal((nlist, D)).astype(F32)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    want = (v - cents[labels]).astype(F32)
    assert np.array_equal(gpu.ivf_residuals(cents, v, labels).view(np.uint32), want.view(np.uint32))
    dev = [torch.from_numpy(a).cuda() for a in (cents, v, labels)]
    assert np.array_equal(gpu.ivf_residuals_torch(*dev).cpu().numpy().view(np.uint32), want.view(np.uint32))
    labels[700] = nlist
    for call in (lambda: gpu.ivf_residuals(cents, v, labels), lambda: gpu.ivf_residuals_torch(dev[0], dev[1], torch.from_numpy(labels).cuda())):
        with pytest.raises(gpu.DpqError) as e:
            call()
        assert e.value.status == ERR_ARG


@pytest.mark.gpu
def test_end_to_end(gpu):
    """train_ivf_centroids -> ivf_assign -> ivf_residuals -> train_codebook -> encode_pq -> DeltaTree -> IVF.from_labels:
    with every list probed, search_residual returns the restatement's ids over the whole index; a second call and the
    non-residual search run on the state it leaves."""
    from deltapq_amd import synth
    n, D, nlist, M, K, k = 4096, 16, 8, 8, 256, 10
    vecs = synth.make_clustered_vectors(n, D, seed=5, n_clusters=40)
    qs = synth.make_clustered_vectors(6, D, seed=6, n_clusters=40, centre_seed=5)
    cents, _ = gpu.train_ivf_centroids(vecs, nlist, max_iters=8)
    vec_labels, _ = gpu.ivf_assign(cents, vecs)
    res = gpu.ivf_residuals(cents, vecs, vec_labels)
    cb, _ = gpu.train_codebook(res, M=M, K=K, max_iters=4)
    codes = gpu.encode_pq(res, cb)
    tree = gpu.DeltaTree(codes, K=K)
    vec_id = tree.vec_id.astype(np.int64)
    c = dict(cb=cb, cents=cents, plain=False)
    entries(c, vec_labels[vec_id], nlist, codes[vec_id])
    every = np.tile(np.arange(nlist, dtype=np.int32), (len(qs), 1))
    with gpu.DeltaPQIndex.open_memory(tree.payload(), n, M, K) as idx:
        idx.set_codebook(cb)
        with gpu.IVF.from_labels(idx, vec_labels[vec_id], nlist, centroids=cents) as ivf:
            got = ivf.search_residual(qs, nlist, k)
            assert np.array_equal(got[0], search(c, qs, every, k)[0])
            assert same(ivf.search_residual(qs, nlist, k), got)
            assert same(ivf.search(qs, nlist, k), ivf.search_probes(qs, every, k))
