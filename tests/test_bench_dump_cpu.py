"""bench.py --dump-outputs: arrays within the budget are written whole, exactly, in float32; a larger one is cut to a seeded
sample of its rows -- the same rows in every run --, with the row numbers beside it, and all files stay within the budget."""
import numpy as np

import bench


def test_arrays_within_the_budget_are_written_whole_and_exact(tmp_path):
    a = np.arange(1 << 16, dtype=np.uint16).reshape(-1, 16)
    b = np.array([0, 1, 255], dtype=np.uint8)
    bench.dump_outputs({"a": a, "b": b}, str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.npy", "b.npy"]
    ga, gb = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert ga.dtype == gb.dtype == np.float32
    assert ga.shape == a.shape and (ga.astype(np.uint16) == a).all() and (gb.astype(np.uint8) == b).all()


def test_a_larger_array_becomes_the_same_sample_of_rows_in_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    big = np.random.default_rng(1).integers(0, 1 << 16, (100_000, 16), dtype=np.uint16)      # 6.4 MB in float32
    for run in ("one", "two"):
        bench.dump_outputs({"big": big, "small": big[:10]}, str(tmp_path / run))
    one, two = tmp_path / "one", tmp_path / "two"
    assert sorted(p.name for p in one.iterdir()) == ["big.npy", "big_rows.npy", "small.npy"]
    assert sum(f.stat().st_size for f in one.iterdir()) <= 1 << 20
    rows = np.load(one / "big_rows.npy")
    assert (rows == np.load(two / "big_rows.npy")).all() and (np.diff(rows) > 0).all() and rows.size > 1000
    got = np.load(one / "big.npy")
    assert got.dtype == np.float32 and (got == big[rows.astype(np.int64)]).all() and (got == np.load(two / "big.npy")).all()
    assert (np.load(one / "small.npy") == big[:10]).all()
