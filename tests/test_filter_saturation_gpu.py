"""The per-(slot, sub-space) saturations of the scan filter on the GPU (M = 8): a 16 384-code bootstrap shard answers batches of
caller-supplied tables (tests/_filter_saturation.py: one batch per class) through both table builders -- the bootstrap
epilogue and, under DPQ_OPT_NO_FUSE_QUANTISE, quantise_kernel -- at 576 queries (nine groups, plain-code
scan with tightening) and 70 (two groups, decode inside the scan), top_k = 1, 10 and 100.

 1. the lists equal the oracle's, ids and distance bits (tests/_option_matrix._rows_equal, as tests/test_numeric_edges.py);
 and, from the first level's tables read back with dpq_debug_filter_tables, for every slot:
 2. sum over m of the row maxima + XMAX XU <= 255 (the m = 0 entries carry the bias): no carry into the neighbour's byte;
 3. every entry <= floor((T - min_m) s) (+ bias at m = 0) in float64 from the slot's threshold, entry by entry (at 576
    queries the rows stand in the scratch's label order: dpq_debug_relabel gives the map);
 4. the saturations equal the restatement's, and the row maxima equal min(SAT_m, row maximum): exactly SAT_m (+ bias) where
    the row's largest fma result reaches it, else that result rounded to nearest, ties to even, as v_cvt_pk_u8_f32 does;
 5. both builders wrote identical tables from identical thresholds.
Assertions 2 - 5 run for every batch size and top_k.  The thresholds and saturations behind the tables are not stored by a
production kernel: the batches run with DPQ_DEV=1, which keeps a copy of the thresholds the first level saw, and the hook
recomputes the saturations from them with the builders' device functions -- so "the saturations equal the restatement's"
pins that function, and the row maxima pin what each builder did with it.
M = 16 keeps its uniform saturation and has no part here.
"""
import ctypes

import numpy as np
import pytest

import _filter_saturation as fs
import _numeric_edges as ne
import _option_matrix as om

N = 16384                     # the smallest shard bootstrap = 1 admits
NQS = (576, 70)
KS = (1, 10, 100)
_handles, _refs = {}, {}


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    yield api
    for idx, _ in _handles.values():
        idx.close()
    _handles.clear()


def _index(api, K, flags):
    """(handle, payload) of the K-centroid shard, one per (K, builder) and module."""
    from deltapq_amd import synth
    if (K, flags) not in _handles:
        payload, _ = synth.encode_dtc(ne.plain_tree(N, 8, K, seed=41))
        _handles[(K, flags)] = (api.DeltaPQIndex.open_memory(payload, N, 8, K, bootstrap=1, flags=flags), payload)
    return _handles[(K, flags)]


def _reference(oracle, name, payload):
    """(tables [576][8][256], K, all distances [576][N]) of a class: computed once, read by every test."""
    if name not in _refs:
        tables, K = fs.class_tables(name, max(NQS))
        alld = np.stack([oracle.scan_lut(payload, N, t[:, :K], 1, want_all=True)[2] for t in tables])
        tables.setflags(write=False)
        alld.setflags(write=False)
        _refs[name] = (tables, K, alld)
    return _refs[name]


def _read_back(idx, n_groups):
    buf = np.empty(n_groups * (fs.NG * fs.M * 256 * 16 + fs.QG * 16), dtype=np.uint8)
    rc = idx._lib.dpq_debug_filter_tables(idx._h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.size)
    assert rc == 0, idx._lib.dpq_last_error()
    return buf


def _label_map(idx):
    """uint8 [M][256] code value -> row of a scratch batch's filter tables, or None where rows are code values."""
    buf = np.empty((fs.M, 256), dtype=np.uint8)
    rc = idx._lib.dpq_debug_relabel(idx._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size)
    assert rc in (0, -7), idx._lib.dpq_last_error()        # -7 = DPQ_ERR_STATE: no label map
    return buf if rc == 0 else None


def _check_tables(raw, tables, nq, what, labels=None):
    n_groups = -(-nq // fs.QG)
    entries, sat, keys = fs.unpack_tables(raw.tobytes(), n_groups)
    if labels is not None:                                  # rows in label order -> rows by code value
        entries = np.take_along_axis(entries, np.broadcast_to(labels.astype(np.int64)[None], entries.shape), axis=2)
    ent = entries.astype(np.int64)
    # 2. no carry: the largest field sum a node can reach, with the tightening's headroom
    top = ent.max(axis=2).sum(axis=1) + fs.XMAX * fs.XU
    assert np.all(top[:nq] <= 255), "%s: field sums up to %d" % (what, top[:nq].max())
    # padding slots reject everything
    assert np.all(entries[nq:, 0] == 255) and np.all(entries[nq:, 1:] == 0), what
    scaled = 0
    for q in range(nq):
        T = tables[q]
        mins = T.min(axis=1)
        s32, bias, B = fs.filter_scale(mins, keys[q])
        want = fs.saturations(T, keys[q])
        assert list(sat[q]) == want, "%s slot %d: saturations %s, restated %s" % (what, q, list(sat[q]), want)
        assert sum(want) <= fs.SAT_BUDGET and max(want) <= fs.SAT_CAP
        if s32 == 0:
            assert np.all(ent[q][np.isfinite(T)] == 0), "%s slot %d: no scale, yet entries" % (what, q)
            continue
        scaled += 1
        # 3. lower bound, in float64 with the exact scale (the kernel's carries a factor 1 - 2^-20 on top)
        tau = np.uint32(int(keys[q]) >> 32).view(np.float32)
        s = fs.QT / (np.float64(tau) * (1.0 + 2.0 ** -20) - B)
        with np.errstate(invalid="ignore", over="ignore"):
            bound = np.floor((T.astype(np.float64) - mins[:, None].astype(np.float64)) * s)
        bound[:, :] = np.where(np.isfinite(bound), bound, 1e18)
        bound[0] += bias
        assert np.all(ent[q] <= bound), "%s slot %d: an entry above its exact value" % (what, q)
        # 4. row maxima
        for m in range(fs.M):
            clamp = want[m] + (bias if m == 0 else 0)
            v = fs.fma32(T[m], s32, fs.filter_offset(s32, bias, mins[m], m))
            v = np.float32(clamp) if np.isnan(v).any() else v.max()          # (+inf x scale: beyond every clamp)
            got = int(ent[q, m].max())
            if v >= clamp:
                assert got == clamp, "%s slot %d row %d: maximum %d, saturation %d" % (what, q, m, got, clamp)
            else:                                                            # v_cvt_pk_u8_f32: to nearest, ties to even
                assert got == max(int(np.rint(v)), 0), "%s slot %d row %d: maximum %d of %r" % (what, q, m, got, v)
    return scaled


@pytest.mark.gpu
@pytest.mark.parametrize("name", fs.CLASSES)
def test_saturated_filter_tables_and_lists(gpu, oracle, monkeypatch, name):
    monkeypatch.setenv("DPQ_DEV", "1")       # dpq_debug_filter_tables is a developer hook
    K = fs.class_tables(name, 1)[1]
    fused, payload = _index(gpu, K, 0)
    unfused, _ = _index(gpu, K, 2)           # DPQ_OPT_NO_FUSE_QUANTISE
    tables, K, alld = _reference(oracle, name, payload)
    pos = np.arange(N, dtype=np.int64)
    rep = om.reported_ids(pos, 0, N)
    scaled = 0
    for nq in NQS:
        t = np.ascontiguousarray(tables[:nq, :, :K])
        for k in KS:
            want = [om.topk_row(alld[q], pos, rep, k) for q in range(nq)]
            raws = []
            for idx, builder in ((fused, "bootstrap epilogue"), (unfused, "quantise kernel")):
                what = "%s nq=%d top-%d, %s" % (name, nq, k, builder)
                om._rows_equal(idx.query_batch_tables(t, k), want, what)                       # 1.
                raws.append(_read_back(idx, -(-nq // fs.QG)))
            # 5. tables, and behind them the thresholds they were built from and the saturations those give
            assert np.array_equal(raws[0], raws[1]), "%s nq=%d top-%d: the builders' tables differ" % (name, nq, k)
            # (576 queries scan the plain-code scratch, whose table rows stand in label order; 70 decode inside the scan)
            labels = _label_map(fused) if nq == 576 else None
            n_scaled = _check_tables(raws[0], tables, nq, "%s nq=%d top-%d" % (name, nq, k), labels)  # 2. - 4.
            print("%s nq=%d top-%d: %d of %d slots have a scale" % (name, nq, k, n_scaled, nq))
            scaled += n_scaled
    assert scaled > 0, "%s: no slot had a scale, the rule never ran" % name
