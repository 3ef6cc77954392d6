"""CPU: bench.py's --full / --dump-outputs options (no GPU launch)."""
import os

import numpy as np
import torch

import bench


def test_plain_run_is_lean_and_full_restores_the_rest():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_verify and a.no_kernel_timing and a.no_cpu_baseline
    f = bench.parse(["--full"])
    assert f.full and not (f.no_verify or f.no_kernel_timing or f.no_cpu_baseline)
    f = bench.parse(["--full", "--no-cpu-baseline", "--dump-outputs", "d"])
    assert f.no_cpu_baseline and not f.no_verify and f.dump_outputs == "d"


def test_dump_outputs_formats_sample_and_budget(tmp_path):
    cap = bench.DUMP_BYTES // 8 // 3
    g = torch.Generator().manual_seed(0)
    outs = {"small_i": torch.arange(-5, 7, dtype=torch.int32).reshape(3, 4),
            "wide_i": torch.tensor([1, (1 << 24) + 1], dtype=torch.int64),
            "big_f": torch.randn(cap + 1000, generator=g)}
    outs["big_f"][3] = float("nan")
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in outs}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in outs)
    assert got["small_i"].dtype == np.float32 and got["small_i"].shape == (3, 4)
    assert np.array_equal(got["small_i"], outs["small_i"].numpy())
    # 2^24 + 1 is not a float32: float64 keeps it
    assert got["wide_i"].dtype == np.float64 and got["wide_i"][1] == (1 << 24) + 1
    # above the cap: a fixed sample of cap elements, the same in every run
    assert got["big_f"].dtype == np.float32 and got["big_f"].shape == (cap,)
    assert np.isin(got["big_f"][~np.isnan(got["big_f"])], outs["big_f"].numpy()).all()
    assert np.array_equal(got["big_f"], np.load(tmp_path / "b" / "big_f.npy"), equal_nan=True)
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
