"""bench.py --dump-outputs without a GPU: dump_outputs() writes float32 arrays, whole when small, a fixed seeded sample with its
positions when large, and stays within its budget."""
import importlib.util
import os

import numpy as np
import torch

import oracle_lib


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(oracle_lib.ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_arrays_are_written_whole(tmp_path):
    bench = load_bench()
    res = torch.tensor([0, 1, 2, 1, 0], dtype=torch.uint8)
    bm = torch.tensor([10], dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path / "out"), {"results": res, "bitmap": bm})
    a, b = np.load(tmp_path / "out" / "results.npy"), np.load(tmp_path / "out" / "bitmap.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert a.tolist() == [0, 1, 2, 1, 0] and b.tolist() == [10]
    assert sorted(os.listdir(tmp_path / "out")) == ["bitmap.npy", "results.npy"]


def test_large_arrays_are_sampled_at_fixed_positions(tmp_path, monkeypatch):
    bench = load_bench()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 1000)
    x = torch.arange(50000, dtype=torch.int64) % 3
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"results": x})
    idx_a, idx_b = np.load(tmp_path / "a" / "results_index.npy"), np.load(tmp_path / "b" / "results_index.npy")
    vals = np.load(tmp_path / "a" / "results.npy")
    assert idx_a.dtype == np.float64 and vals.dtype == np.float32 and vals.shape == (1000,)
    assert np.array_equal(idx_a, idx_b) and np.all(np.diff(idx_a) > 0)
    assert np.array_equal(vals, (idx_a.astype(np.int64) % 3).astype(np.float32))
    # a later, smaller dump into the same folder is whole: no stale positions are left beside it
    bench.dump_outputs(str(tmp_path / "a"), {"results": x[:10]})
    assert not os.path.exists(tmp_path / "a" / "results_index.npy")


def test_budget_of_a_full_dump():
    bench = load_bench()
    assert 2 * bench.DUMP_MAX_ELEMENTS * (4 + 8) <= 64 * 2 ** 20
