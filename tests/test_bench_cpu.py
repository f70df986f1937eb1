"""bench.py --dump-outputs: what the timed path computed, written as float64 .npy files under a size bound; --full: the legs beside
the headline (roofline pass, CPU baseline) run only when asked for."""
import os

import numpy as np

import bench


def _outputs(n):
    return {"loglik": np.linspace(-900.0, -800.0, n), "info": np.arange(n, dtype=np.int32) % 3, "probabilities": np.full(n, 1.0 / n)}


def test_dump_writes_every_array_whole_as_float64(tmp_path):
    arrays = _outputs(1000)
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["info.npy", "loglik.npy", "probabilities.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)


def test_dump_above_the_bound_keeps_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    arrays = _outputs(20000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
        files = os.listdir(tmp_path / run)
        assert sorted(files) == ["index.npy", "info.npy", "loglik.npy", "probabilities.npy"]
        assert sum(os.path.getsize(tmp_path / run / f) for f in files) <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "index.npy")) and len(np.unique(idx)) == len(idx) > 0
    for name, a in arrays.items():
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), a[idx.astype(np.int64)].astype(np.float64))


def test_extra_legs_only_with_full():
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not plain.full and plain.steps == 3 and plain.warmup == 1
    full = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert full.full and not full.no_roofline and not full.no_cpu_baseline
