"""bench.py --dump-outputs: the files it writes (float64 .npy, within the size limit, a fixed sample of
an output too large for it).  No GPU: the writer is called on host arrays; tests/test_gpu_bench_workload.py
runs the whole command."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_written_whole_in_float64(tmp_path):
    x = np.random.RandomState(1).standard_normal(2048)
    bench.dump_outputs(str(tmp_path / "d"), {"x": x, "y": x[:10].astype(np.float32)})
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x)
    y = np.load(tmp_path / "d" / "y.npy")
    assert y.dtype == np.float64 and np.array_equal(y, x[:10].astype(np.float32))


def test_large_output_is_a_fixed_sample_within_the_limit(tmp_path):
    limit = 64 << 10
    x = np.arange(100000, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "z": -x}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in ("x.npy", "z.npy"))
    assert total <= limit
    xa, xb, za = (np.load(tmp_path / d / f) for d, f in (("a", "x.npy"), ("b", "x.npy"), ("a", "z.npy")))
    assert np.array_equal(xa, xb)                      # the same entries on every run
    assert np.all(np.diff(xa) > 0) and np.array_equal(za, -xa)   # sorted indices, one draw per output
    assert xa.size > 1000


def test_default_limit_is_64_mb():
    assert bench.DUMP_BYTES_MAX == 64 * 1024 * 1024
