"""CPU only: bench.py --dump-outputs writes float32 .npy files of what the timed path returned, within 64 MB, and takes the same
seeded sample of items from every array when the outputs are larger - so that two builds compare output for output."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    count = 1000
    status = (np.arange(count) % 3 == 0).astype(np.uint8)
    resp = np.random.default_rng(1).integers(0, 256, size=(5, count, 32), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"status": (status, 0), "responses": (resp, 1)}, count)
    assert sorted(os.listdir(tmp_path)) == ["responses.npy", "status.npy"]
    s, r = np.load(tmp_path / "status.npy"), np.load(tmp_path / "responses.npy")
    assert s.dtype == r.dtype == np.float32 and np.array_equal(s, status) and np.array_equal(r, resp)


def test_large_outputs_keep_one_fixed_sample_of_items_under_the_budget(tmp_path):
    count, budget = 1 << 16, 1 << 20
    t = np.random.default_rng(2).integers(0, 256, size=(count, 32), dtype=np.uint8)
    resp = np.random.default_rng(3).integers(0, 256, size=(4, count, 32), dtype=np.uint8)
    status = np.zeros(count, np.uint8)
    arrays = {"t": (t, 0), "responses": (resp, 1), "status": (status, 0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, count, "rank1_", budget)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rank1_responses.npy", "rank1_sample_index.npy", "rank1_status.npy", "rank1_t.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= budget + 4 * 128   # (+ the .npy headers)
    idx = np.load(tmp_path / "a" / "rank1_sample_index.npy").astype(np.int64)
    assert idx.size > 0 and np.all(np.diff(idx) > 0) and idx[-1] < count
    assert np.array_equal(np.load(tmp_path / "a" / "rank1_t.npy"), t[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "rank1_responses.npy"), resp[:, idx])
    for n in names:   # the same arguments, the same files
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
