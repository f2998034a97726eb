"""bench.py's --dump-outputs writer (no GPU): names, dtype, the 64 MB bound and
the run-to-run identity of the seeded sample."""

import os

import numpy as np

import bench


def test_dump_outputs_small_arrays_whole(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = np.linspace(0.0, 1.0, 7)
    bench.dump_outputs(str(tmp_path / "o"), {"reverse": a, "forward": b})
    assert sorted(os.listdir(tmp_path / "o")) == ["forward.npy", "reverse.npy"]
    ra, rb = np.load(tmp_path / "o" / "reverse.npy"), np.load(tmp_path / "o" / "forward.npy")
    assert ra.dtype == np.float64 and ra.shape == (3, 4) and np.array_equal(ra, a)
    assert rb.dtype == np.float64 and np.array_equal(rb, b)


def test_dump_outputs_bounded_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(5000, dtype=np.float64).reshape(50, 100)     # 40 kB > its 2 kB share
    small = np.ones(10)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert np.array_equal(x, y)                                   # the same sample every run
    assert x.shape == (256,) and np.all(np.diff(x) > 0)           # 2048 B of distinct elements, in order
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small)
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert total <= 4096 + 2 * 128                                # payload bound + the two .npy headers
