"""CPU: bench.py --dump-outputs -- the writer alone, on host tensors: float32 files, the 64 MB cap, and the same env rows on
every run of the same shape."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _outs(N, G):
    import torch
    g = torch.Generator().manual_seed(3)
    return {"obs": torch.randint(0, 16, (N, G, G), dtype=torch.int32, generator=g),
            "reward": torch.randn(N, generator=g), "done": torch.rand(N, generator=g) < 0.3}


def test_every_env_when_it_fits(tmp_path):
    import bench
    outs = _outs(300, 8)
    d = bench.dump_outputs(str(tmp_path), outs, 300)
    assert d["envs"] == d["of"] == 300 and sorted(d["files"]) == ["done.npy", "env_index.npy", "obs.npy", "reward.npy"]
    for name, t in outs.items():
        a = np.load(str(tmp_path / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert (a == t.numpy().astype(np.float32)).all(), name
    idx = np.load(str(tmp_path / "env_index.npy"))
    assert idx.dtype == np.float64 and (idx == np.arange(300)).all()


def test_a_fixed_sample_when_it_does_not_fit(tmp_path):
    import bench
    outs = _outs(5000, 11)
    budget = 200 * (8 + 4 * (121 + 2))
    a = bench.dump_outputs(str(tmp_path / "a"), outs, 5000, budget=budget)
    b = bench.dump_outputs(str(tmp_path / "b"), outs, 5000, budget=budget)
    assert a["envs"] == b["envs"] == 200 and a["of"] == 5000
    idx = np.load(str(tmp_path / "a" / "env_index.npy")).astype(np.int64)
    assert len(np.unique(idx)) == 200 and (np.diff(idx) > 0).all() and idx[-1] < 5000
    for f in a["files"]:
        assert open(str(tmp_path / "a" / f), "rb").read() == open(str(tmp_path / "b" / f), "rb").read(), f
    for name, t in outs.items():
        assert (np.load(str(tmp_path / "a" / (name + ".npy"))) == t.numpy()[idx].astype(np.float32)).all(), name


@pytest.mark.parametrize("shape", [(1 << 20, (11, 11)), (1 << 20, (32, 32)), (1 << 20, (5, 5, 5))])
def test_metric_sizes_stay_under_64_mb(tmp_path, shape):
    import bench
    import torch
    N, row = shape
    outs = {"obs": torch.zeros((1,) + row).expand((N,) + row), "obs_local": torch.zeros(1, 4, 5, 5).expand(N, 4, 5, 5),
            "reward": torch.zeros(1).expand(N), "done": torch.zeros(1, dtype=torch.bool).expand(N)}
    d = bench.dump_outputs(str(tmp_path), outs, N)
    assert 0 < d["envs"] < N
    assert sum(os.path.getsize(str(tmp_path / f)) for f in d["files"]) <= 64 * 10 ** 6


def test_steps_must_be_positive():
    import bench
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7
    assert bench.parse_args(["--dump-outputs", "x"]).dump_outputs == "x"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
