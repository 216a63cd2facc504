"""CPU tests of bench.py's command line and its --dump-outputs writer (no GPU work)."""
import sys

import numpy as np
import pytest
import torch


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.gpus) == (7, 2, 1)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_options(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--full", "--no-pmc", "--dump-outputs", str(tmp_path))
    assert a.full is True and a.no_pmc is True and a.dump_outputs == str(tmp_path)


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import bench
    y = torch.arange(6, dtype=torch.float64).reshape(3, 2).requires_grad_(True)
    f = torch.arange(12, dtype=torch.float16).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"y": y, "neg_dy": f}, 0)
    bench.dump_outputs(str(tmp_path / "d"), {"y": y}, 1)
    got = np.load(tmp_path / "d" / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y.detach().numpy())
    got = np.load(tmp_path / "d" / "neg_dy.npy")
    assert got.dtype == np.float32 and np.array_equal(got, f.float().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "y_rank1.npy"), y.detach().numpy())


def test_dump_outputs_samples_an_array_over_its_share(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 400)  # two arrays: 100 float32 values each
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    small = torch.ones(5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, 0)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and a.dtype == np.float32
    assert np.array_equal(a, b)  # the same seeded index set on every run
    assert np.all(np.diff(a) > 0)  # distinct elements of the input, in ascending position
    assert np.load(tmp_path / "a" / "small.npy").shape == (5,)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= 2 * 400 + 2 * 128  # payload within the cap (+ the npy headers)
