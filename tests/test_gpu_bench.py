"""GPU: bench.py --dump-outputs writes the outputs of the LAST timed step:
each workload's last_outputs() after warm-up + timed steps equals a fresh
single-step run of the batch that step read, and dump_outputs() stores them
unchanged (small shapes, in process)."""
import os

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu


def run_workload(dev, argv):
    args = bench.parse(argv)
    wl = bench.WORKLOADS[args.workload](args, dev, 0, 1)
    wl.prepare_timing()
    wl.run(args.warmup, timed=False)
    torch.cuda.synchronize(dev)
    wl.run(args.steps, timed=True)
    torch.cuda.synchronize(dev)
    return args, wl, {k: v.clone() for k, v in wl.last_outputs().items()}


def same(a, b):
    return torch.equal(a, b) or torch.allclose(a, b, equal_nan=True)


@pytest.mark.parametrize("workload,pairs", [("extract", False), ("pairs", True)])
def test_extract_last_outputs_are_the_last_steps(dev, tmp_path, workload, pairs):
    # 2 warm-up + 4 timed steps over a ring of 3: the last step is step 5,
    # which reads batch 5 % 3 = 2 and writes ring set 2
    args, wl, last = run_workload(dev, [
        "--workload", workload, "--batch", "4", "--points", "1024", "--channels", "16",
        "--k", "32", "--res", "32", "--batches", "3", "--warmup", "2", "--steps", "4"])
    ref = wl.ex.forward(*wl.batches[2])
    torch.cuda.synchronize(dev)
    keys = ["knn_idx", "local_ppf", "norm_coords", "ind", "cnt", "grid", "devox", "desc",
            "dinds", "dwgts"] + (["corr12", "corr21", "idx1", "idx2", "count"] if pairs else [])
    assert sorted(last) == sorted(keys)
    for key in keys:
        assert same(last[key], ref[key]), key
    other = wl.ex.forward(*wl.batches[1])
    assert not torch.equal(last["knn_idx"], other["knn_idx"])

    bench.dump_outputs(last, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in keys)
    cap = bench.DUMP_BYTES // 8 // len(keys)
    total = 0
    for key in keys:
        a = np.load(tmp_path / (key + ".npy"))
        total += a.nbytes
        assert a.dtype == np.float32
        full = last[key].cpu().numpy()
        if full.size <= cap:
            assert a.shape == full.shape and np.array_equal(a, full, equal_nan=True), key
        else:
            pos = np.sort(np.random.default_rng(20240).integers(0, full.size, cap))
            assert np.array_equal(a, full.reshape(-1)[pos].astype(np.float32), equal_nan=True), key
    assert total <= 64 * 1000 * 1000


def test_c3_last_outputs_are_the_last_steps(dev):
    # 1 warm-up call of 2 steps, then a timed call of 3: its last step is
    # step 2 of that call, batch 2 % 4 = 2
    args, wl, last = run_workload(dev, [
        "--workload", "c3", "--batch", "4", "--points", "1024", "--channels", "16",
        "--k", "32", "--res", "16", "--batches", "4", "--warmup", "2", "--steps", "3"])
    ref = []
    wl._serial(1, False, ref, first=2)
    torch.cuda.synchronize(dev)
    out, (gg, gx) = ref[0]
    for key in ("knn_idx", "local_ppf", "norm_coords", "ind", "cnt", "grid", "devox", "desc",
                "dinds", "dwgts"):
        assert same(last[key], out[key]), key
    assert torch.equal(last["grad_grid"], gg)
    assert torch.equal(last["grad_x"], gx)


def test_c5_last_outputs_are_the_steps(dev):
    args, wl, last = run_workload(dev, [
        "--workload", "c5", "--batch", "2", "--points", "4096", "--channels", "8",
        "--k", "16", "--res", "16", "--warmup", "1", "--steps", "2"])
    ref = wl._step_outputs()
    torch.cuda.synchronize(dev)
    assert set(ref) <= set(last)
    for key, v in ref.items():
        assert torch.equal(last[key].view(torch.int32), v.view(torch.int32)), key
