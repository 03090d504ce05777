"""bench.py --dump-outputs: the writer's file format and size cap (no GPU).  The end-to-end run on a GPU is
tests/test_gpu_parity.py::test_bench_one_gpu_times_steps_and_dumps_the_last_one."""
import os

import numpy as np

import bench


def _lists(nq, k, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 2**31 - 1, (nq, k), dtype=np.int32)
    dists = np.sort(rng.random((nq, k), dtype=np.float32), axis=1)
    return ids, dists


def test_dump_outputs_writes_the_whole_result_as_float(tmp_path):
    ids, dists = _lists(10, 7, seed=1)
    s = bench.dump_outputs(str(tmp_path), ids, dists)
    assert sorted(os.listdir(tmp_path)) == ["dists.npy", "ids.npy"] and not s["rows_sampled"] and s["rows"] == 10
    got_i, got_d = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "dists.npy")
    assert got_i.dtype == np.float64 and got_d.dtype == np.float32
    assert np.array_equal(got_i.astype(np.int64), ids) and np.array_equal(got_d.view(np.uint32), dists.view(np.uint32))


def test_dump_outputs_above_the_cap_writes_a_seeded_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    ids, dists = _lists(300, 50, seed=2)                       # 180 000 B of lists
    runs = []
    for d in ("a", "b"):
        out = str(tmp_path / d)
        s = bench.dump_outputs(out, ids, dists)
        assert s["rows_sampled"] and sorted(os.listdir(out)) == ["dists.npy", "ids.npy", "rows.npy"]
        assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 40_000
        rows = np.load(os.path.join(out, "rows.npy"))
        assert rows.dtype == np.float64 and len(rows) == s["rows"] > 0 and np.all(np.diff(rows) > 0)
        r = rows.astype(np.int64)
        assert np.array_equal(np.load(os.path.join(out, "ids.npy")).astype(np.int64), ids[r])
        assert np.array_equal(np.load(os.path.join(out, "dists.npy")), dists[r])
        runs.append(r)
    assert np.array_equal(runs[0], runs[1])                     # the same rows every time
