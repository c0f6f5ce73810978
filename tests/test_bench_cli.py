"""CPU: the benchmark's command line (a plain run by default, the further measurements behind
--full) and the --dump-outputs writer (float32 .npy files, a fixed sample within the byte budget)."""
import os

import numpy as np
import pytest
import torch


def test_plain_run_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    b = bench.parse(["--full", "--dump-outputs", "somewhere", "--no-pmc"])
    assert b.full and b.dump_outputs == "somewhere" and b.no_pmc
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_whole_small_arrays_as_float32(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    outs = [(c, torch.randn(1, 2, 37, 8, generator=g).bfloat16()) for c in (4, 5)]
    info = bench.dump_outputs(str(tmp_path / "d"), outs, 2)
    assert sorted(info) == ["out_call004_set0", "out_call005_set1"]
    for (c, t), name in zip(outs, sorted(info)):
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == np.float32 and not info[name]["sampled"]
        assert np.array_equal(a, t.float().reshape(-1).numpy())
        assert info[name]["shape"] == [1, 2, 37, 8]


def test_dump_outputs_samples_large_arrays_reproducibly(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * 100)      # 100 elements per array
    t = torch.arange(5000, dtype=torch.float32).reshape(1, 1, 500, 10)
    outs = [(0, t), (1, t + 0.5)]
    bench.dump_outputs(str(tmp_path / "a"), outs, 2)
    bench.dump_outputs(str(tmp_path / "b"), outs, 2)
    total = 0
    for name in ("out_call000_set0.npy", "out_call001_set1.npy"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == (100,)
        assert np.array_equal(a, b)                                    # same sample every run
        total += os.path.getsize(tmp_path / "a" / name)
    first = np.load(tmp_path / "a" / "out_call000_set0.npy")
    second = np.load(tmp_path / "a" / "out_call001_set1.npy")
    assert np.array_equal(second, first + 0.5)                         # same indices in every array
    assert np.all(np.diff(first) >= 0) and len(np.unique(first)) > 90  # spread over the array
    assert total <= 4 * 2 * 100 + 2 * 256                              # payload + .npy headers
