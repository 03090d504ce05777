"""The resident plain-code image: a shard that one tile holds is decoded ONCE per handle, by the first batch that scans
the plain codes, and every later batch, on either pipeline lane and through every entry point, reads that image.  All
comparisons are bit for bit: ids, and distances viewed as uint32."""
import numpy as np
import pytest

from conftest import assert_parity, make_case, oracle_topk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def assert_same(a, b, what):
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])), what + ": ids differ"
    assert np.array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32)), what + ": distances differ"


def assert_range_same(a, b, what):
    for x, y, name in zip(a, b, ("lims", "ids", "dists")):
        if name == "dists":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differ" % (what, name)


def three_profiled_batches(gpu, payload, n, cb, qs, k, **kw):
    """Three identical batches on one fresh handle: [(ids, dists, profile of that batch alone)]."""
    out = []
    with gpu.DeltaPQIndex.open_memory(payload, n, cb.shape[0], 256, **kw) as idx:
        idx.set_codebook(cb)
        idx.profile_enable(True)
        for _ in range(3):
            idx.profile_reset()
            ids, dists = idx.query_batch(qs, k)
            out.append((ids, dists, idx.profile_read()))
    return out


def check_one_decode_per_handle(runs):
    (_, _, p0), (_, _, p1), (_, _, p2) = runs
    assert p0["decode_ms"] > 0.0 and p0["scan_launches"] > 0, p0
    for p in (p1, p2):
        assert p["decode_ms"] == 0.0 and p["scan_launches"] > 0, p
    assert_same(runs[0], runs[1], "second batch")
    assert_same(runs[0], runs[2], "third batch")


def test_one_decode_per_handle(gpu, oracle, codebook):
    """70 001 codes in 4-chunk segments, bootstrap on, 200 queries (four groups), top-40: the first batch of a handle
    decodes, the next two do not and give the same lists; a tiled scratch (37 segments of 274) still decodes per batch."""
    from deltapq_amd import synth
    n, k = 70_001, 40
    _, payload, _ = make_case(n, seed=45)
    qs = synth.make_queries(200, 128, seed=46)
    runs = three_profiled_batches(gpu, payload, n, codebook, qs, k, chunks_per_segment=4, bootstrap=1)
    check_one_decode_per_handle(runs)
    assert_parity(runs[0][0][:8], runs[0][1][:8], oracle_topk(oracle, payload, n, codebook, qs[:8], k), n)
    tiled = three_profiled_batches(gpu, payload, n, codebook, qs, k, chunks_per_segment=4, bootstrap=1, batch_decode=37)
    for i, (_, _, p) in enumerate(tiled):
        assert p["decode_ms"] > 0.0 and p["scan_launches"] > 0, (i, p)
        assert_same(tiled[i], runs[0], "tiled batch %d" % i)


def test_one_decode_per_handle_m16(gpu, oracle):
    """The same for M = 16 (4-dword codes; 130 queries are five groups of 32): 150 000 codes, top-30."""
    from deltapq_amd import synth
    n, k = 150_000, 30
    cb16 = synth.make_codebook(16, 256, 8, seed=3)
    payload, _ = synth.encode_dtc(synth.synth_tree(n, 16, seed=77, mean_diffs=5.0))
    qs = synth.make_queries(130, 128, seed=78)
    runs = three_profiled_batches(gpu, payload, n, cb16, qs, k, bootstrap=1)
    check_one_decode_per_handle(runs)
    assert_parity(runs[0][0][:8], runs[0][1][:8], oracle_topk(oracle, payload, n, cb16, qs[:8], k), n)
    tiled = three_profiled_batches(gpu, payload, n, cb16, qs, k, bootstrap=1, batch_decode=37)
    for i, (_, _, p) in enumerate(tiled):
        assert p["decode_ms"] > 0.0 and p["scan_launches"] > 0, (i, p)
        assert_same(tiled[i], runs[0], "tiled batch %d" % i)


def test_image_survives_everything_else_on_the_handle(gpu, codebook):
    """One handle: a 200-query batch, a 64-query batch (decode inside the scan), one query (stream pass), a filtered
    200-query batch, a range search, another codebook and back, the first batch again.  Every step equals the same call
    on a fresh handle, and the last equals the first."""
    from deltapq_amd import synth
    from deltapq_amd.api import IdFilter
    n, k = 70_001, 40
    _, payload, _ = make_case(n, seed=47)
    qs = synth.make_queries(200, 128, seed=48)
    cb2 = synth.make_codebook(8, 256, 16, seed=99)
    mask = np.random.default_rng(49).random(n + 1) < 0.5

    def opened(cb=codebook):
        idx = gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, chunks_per_segment=4, bootstrap=1)
        idx.set_codebook(cb)
        return idx

    def filtered(idx):
        with IdFilter.from_mask(idx, mask) as f:
            return idx.query_batch_filtered(qs, k, f)

    with opened() as idx:
        first = idx.query_batch(qs, k)
        radius = np.nextafter(first[1][:, 9], np.float32(np.inf))  # the ten nearest codes, tie groups included
        steps = [
            ("64 queries", lambda i: i.query_batch(qs[:64], k), assert_same, codebook),
            ("one query", lambda i: i.query_batch(qs[:1], k), assert_same, codebook),
            ("filtered", filtered, assert_same, codebook),
            ("range search", lambda i: i.range_search(qs, radius), assert_range_same, codebook),
        ]
        got = [(what, call(idx), call, same, cb) for what, call, same, cb in steps]
        idx.set_codebook(cb2)
        got.append(("second codebook", idx.query_batch(qs, k), lambda i: i.query_batch(qs, k), assert_same, cb2))
        idx.set_codebook(codebook)
        again = idx.query_batch(qs, k)
    assert_same(again, first, "the first batch again")
    with opened() as fresh:
        assert_same(first, fresh.query_batch(qs, k), "200 queries against a fresh handle")
    for what, res, call, same, cb in got:
        with opened(cb) as fresh:
            same(res, call(fresh), what + " against a fresh handle")
    lims = got[3][1][0]
    assert lims[-1] >= 10 * len(qs)  # (the range search was no empty one)


@pytest.fixture(scope="module")
def laned_case(gpu, codebook):
    """20 000 codes (bootstrap on), five distinct 200-query sets and the synchronous answers, top-20, of each set and of
    its first 130 queries."""
    from deltapq_amd import synth
    n, k = 20_000, 20
    _, payload, _ = make_case(n, seed=51)
    sets = [synth.make_queries(200, 128, seed=60 + i) for i in range(5)]
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, bootstrap=1) as idx:
        idx.set_codebook(codebook)
        sync = {(i, nq): idx.query_batch(s[:nq], k) for i, s in enumerate(sets) for nq in (200, 130)}
    return dict(n=n, k=k, payload=payload, sets=sets, sync=sync)


def laned_round(gpu, codebook, c, sizes):
    """Enqueues len(sizes) laned batches, cycling the query sets, each with its own outputs; checks every one after
    finish() against the synchronous answer."""
    import torch
    k = c["k"]
    dev = torch.device("cuda:0")
    d_sets = [torch.from_numpy(s).to(dev) for s in c["sets"]]
    with gpu.DeltaPQIndex.open_memory(c["payload"], c["n"], 8, 256, bootstrap=1) as idx:
        idx.set_codebook(codebook)
        outs = []
        for j, nq in enumerate(sizes):
            q = d_sets[j % 5][:nq].contiguous()
            outs.append((q,) + tuple(idx.query_batch_torch(q, k, wait=False)))
        idx.finish()
        torch.cuda.synchronize()
        for j, nq in enumerate(sizes):
            assert_same((outs[j][1].cpu().numpy(), outs[j][2].cpu().numpy()), c["sync"][(j % 5, nq)],
                        "laned batch %d (%d queries)" % (j, nq))


def test_twelve_laned_batches_equal_sizes(gpu, codebook, laned_case):
    laned_round(gpu, codebook, laned_case, [200] * 12)


def test_twelve_laned_batches_alternating_sizes(gpu, codebook, laned_case):
    """200 and 130 queries in turn: neighbours in flight differ in slot count and table extent."""
    laned_round(gpu, codebook, laned_case, [200, 130] * 6)


def test_eight_host_async_batches(gpu, codebook, laned_case):
    c, k = laned_case, laned_case["k"]
    sizes = [200, 130] * 4
    with gpu.DeltaPQIndex.open_memory(c["payload"], c["n"], 8, 256, bootstrap=1) as idx:
        idx.set_codebook(codebook)
        bufs = []
        for j, nq in enumerate(sizes):
            q = np.ascontiguousarray(c["sets"][j % 5][:nq])
            ids, dists = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32)
            bufs.append((q, ids, dists))
            idx.query_batch_host_async(q, k, ids, dists)
        idx.finish()
    for j, nq in enumerate(sizes):
        assert_same(bufs[j][1:], c["sync"][(j % 5, nq)], "host-async batch %d (%d queries)" % (j, nq))


def test_first_use_on_two_streams(gpu, codebook, laned_case):
    """The very first two batches of a fresh handle are laned: the first decodes the image on its lane's stream, the second,
    on the other lane, has to wait for it."""
    laned_round(gpu, codebook, laned_case, [200, 200])
