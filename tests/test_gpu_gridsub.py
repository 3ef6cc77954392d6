"""GPU: ops.grid_subsample / pcr_grid_subsample against the numpy restatement
(tests/gridsub_restate.py) with exact equality -- ints and floats, origin and
dims too; floats are compared as bit patterns.  The contract fixes every
operation and its order, so the tolerance is zero.

Every output buffer and the workspace are poisoned before each call (the C
ABI is called on buffers the test fills), so a slot left unwritten fails.

Size thresholds of the implementation (csrc/gridsub.hip), each tested on both
sides:
  - kGsTile = 1024 points per sort / scan tile: n = 1024 and 1025 (one and two
    tiles), 2049 (three)
  - the bounds kernel takes more than one point per thread past
    kGsBoundsBlocks * 256 = 16384 points: n = 16384 and 16385
  - sort passes of 8 key bits, the result's buffer alternating with their
    number: 0 passes (one cell), 1, 2, 3 and all 8 (keys past 2^32)
  - the sum's batches of 32 points, then of eight, then single points: cells
    of 1, 7, 8, 9, 31, 32, 33, 40, 41, 64 and 73 points
  - the sum's workgroup takes 64 slots (n = 63, 64, 65) and CW = 4, 8, 16, 32
    or 64 channels of the 3 + c, in chunks of 64 past that: c = 1 | 2, 5 | 6,
    13 | 14, 29 | 30, 61 | 62 are the two sides of each step (3 + c = 4 | 5,
    8 | 9, 16 | 17, 32 | 33, 64 | 65); the transpose to point-major rows has
    the same 64 x 64 tiles
  - the largest supported cloud, n = 262144
"""
import numpy as np
import pytest
import torch

import gridsub_restate as gr

pytestmark = pytest.mark.gpu
F = np.float32


def run_gpu(dev, xyz, cell, features=None, counts=None):
    """pcr_grid_subsample on poisoned outputs and a poisoned workspace ->
    the dict of ops.grid_subsample as numpy"""
    from pcr_amd import _lib
    lib = _lib.load()
    b, _, n = xyz.shape
    c = 0 if features is None else features.shape[1]
    tx = torch.from_numpy(np.ascontiguousarray(xyz, F)).to(dev)
    tf = None if features is None else torch.from_numpy(np.ascontiguousarray(features, F)).to(dev)
    tc = None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).to(dev)

    def poison_f(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)

    def poison_i(*shape):
        return torch.full(shape, -7777, dtype=torch.int32, device=dev)
    out = dict(xyz=poison_f(b, 3, n), features=None if tf is None else poison_f(b, c, n),
               count=poison_i(b), cell_of=poison_i(b, n), cell_count=poison_i(b, n),
               origin=poison_f(b, 3), dims=poison_i(b, 3), status=poison_i(b))
    ws = torch.full((max(256, lib.pcr_grid_subsample_workspace_size(b, n, c)),), 0xAB,
                    dtype=torch.uint8, device=dev)

    def ptr(t):
        return None if t is None or t.numel() == 0 else t.data_ptr()
    _lib.check(lib.pcr_grid_subsample(
        ptr(tx), ptr(tf), ptr(tc), b, n, c, float(cell), ptr(out["xyz"]), ptr(out["features"]),
        ptr(out["count"]), ptr(out["cell_of"]), ptr(out["cell_count"]), ptr(out["origin"]),
        ptr(out["dims"]), ptr(out["status"]), ptr(ws), ws.numel(),
        torch.cuda.current_stream().cuda_stream), "grid_subsample")
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def check_consistent(got, n, counts=None):
    """cell_count sums to the valid count and cell_of is a valid map"""
    b = got["count"].shape[0]
    for q in range(b):
        m = n if counts is None else int(counts[q])
        cells = int(got["count"][q])
        if got["status"][q] != 0:
            assert cells == 0 and (got["cell_of"][q] == -1).all()
            assert not got["cell_count"][q].any() and not got["xyz"][q].any()
            continue
        assert 1 <= cells <= m
        assert got["cell_count"][q, :cells].sum() == m and (got["cell_count"][q, :cells] >= 1).all()
        assert not got["cell_count"][q, cells:].any()
        of = got["cell_of"][q]
        assert (of[:m] >= 0).all() and (of[:m] < cells).all() and (of[m:] == -1).all()
        assert np.array_equal(np.bincount(of[:m], minlength=n), got["cell_count"][q])


@pytest.fixture(scope="module")
def shapes():
    """(b, n, c) -> (inputs, restatement), computed once"""
    cache = {}

    def get(b, n, c, cell=0.35, seed=0):
        key = (b, n, c, cell, seed)
        if key not in cache:
            rng = np.random.default_rng(1000 * seed + 7 * n + b + 31 * c)
            xyz = rng.standard_normal((b, 3, n)).astype(F)
            xyz += rng.uniform(-3, 3, (b, 3, 1)).astype(F)
            feat = rng.standard_normal((b, c, n)).astype(F) if c else None
            cache[key] = (xyz, feat, gr.grid_subsample_batch(xyz, cell, feat))
        return cache[key]
    return get


@pytest.mark.parametrize("b,n,c", [
    (1, 1, 0), (3, 1, 3), (33, 2, 1), (1, 2, 67), (3, 63, 0), (1, 64, 1), (33, 64, 3),
    (3, 65, 67), (1, 65, 3), (1, 1000, 0), (3, 1000, 1), (33, 1000, 3), (1, 1000, 67),
    # the tile threshold (kGsTile = 1024), either side, and three tiles
    (3, 1024, 3), (3, 1025, 3), (1, 2049, 1)])
def test_matches_the_restatement(dev, shapes, b, n, c):
    xyz, feat, exp = shapes(b, n, c)
    got = run_gpu(dev, xyz, 0.35, feat)
    gr.assert_same(got, exp, (b, n, c))
    assert (got["status"] == 0).all()
    check_consistent(got, n)


@pytest.mark.parametrize("c", [1, 2, 5, 6, 13, 14, 29, 30, 61, 62, 130])
def test_channel_widths(dev, shapes, c):
    """either side of every channel-width step of the sum kernel"""
    xyz, feat, exp = shapes(2, 200, c, 0.6, seed=2)
    got = run_gpu(dev, xyz, 0.6, feat)
    gr.assert_same(got, exp, c)
    check_consistent(got, 200)


@pytest.mark.parametrize("n", [16384, 16385])
def test_bounds_kernel_threshold(dev, n):
    """kGsBoundsBlocks * 256 = 16384: the last point (the one a missing
    grid-stride step would skip) carries the minimum and the maximum"""
    rng = np.random.default_rng(n)
    xyz = rng.standard_normal((1, 3, n)).astype(F)
    xyz[0, :, n - 1] = (-9.0, 9.5, -9.25)
    xyz[0, 1, n - 2] = -9.75
    exp = gr.grid_subsample_batch(xyz, 1.5)
    got = run_gpu(dev, xyz, 1.5)
    gr.assert_same(got, exp, n)
    check_consistent(got, n)


@pytest.mark.parametrize("cell,shift,passes", [(100.0, 50.0, 0), (2.0, 0.0, 1), (0.4, 0.0, 2),
                                               (0.1, 0.0, 3), (0.02, 0.0, 4)])
def test_sort_pass_counts(dev, cell, shift, passes):
    """0 to 4 radix passes (the sorted data ends in either buffer)"""
    rng = np.random.default_rng(5)
    xyz = (rng.uniform(-4, 4, (2, 3, 1500)) + shift).astype(F)
    feat = rng.standard_normal((2, 2, 1500)).astype(F)
    exp = gr.grid_subsample_batch(xyz, cell, feat)
    bits = [int(np.prod(d.astype(np.int64)) - 1).bit_length() for d in exp["dims"]]
    assert all((v + 7) // 8 == passes for v in bits), bits
    got = run_gpu(dev, xyz, cell, feat)
    gr.assert_same(got, exp, cell)
    check_consistent(got, 1500)


@pytest.mark.parametrize("name", list(gr.edge_clouds()))
def test_edge_clouds(dev, name):
    """one cell (n = 70, 1500), every point its own cell, duplicates, negative
    coordinates, points on faces, the clamp case, signed zeros, 64-bit keys,
    cells of 1 .. 73 points"""
    xyz, feat, cell = gr.edge_clouds()[name]
    n = xyz.shape[1]
    exp = gr.grid_subsample_batch(xyz[None], cell, None if feat is None else feat[None])
    got = run_gpu(dev, xyz[None], cell, None if feat is None else feat[None])
    gr.assert_same(got, exp, name)
    check_consistent(got, n)
    if name.startswith("one_cell"):
        assert got["count"][0] == 1
    if name == "own_cell":
        assert got["count"][0] == n
    if name == "keys64":
        assert np.prod(got["dims"][0].astype(np.int64)) > 1 << 32


def test_ragged_counts(dev):
    """counts n, 1, 0 and n + 1: the last two give status 1"""
    n = 300
    rng = np.random.default_rng(11)
    xyz = rng.standard_normal((4, 3, n)).astype(F)
    feat = rng.standard_normal((4, 3, n)).astype(F)
    counts = np.array([n, 1, 0, n + 1], np.int32)
    exp = gr.grid_subsample_batch(xyz, 0.4, feat, counts)
    got = run_gpu(dev, xyz, 0.4, feat, counts)
    gr.assert_same(got, exp, "ragged")
    assert got["status"].tolist() == [0, 0, 1, 1] and got["count"][1] == 1
    check_consistent(got, n, np.array([n, 1, 0, 0]))
    # a ragged batch across a tile boundary
    n = 1100
    xyz = rng.standard_normal((3, 3, n)).astype(F)
    counts = np.array([1100, 1024, 37], np.int32)
    exp = gr.grid_subsample_batch(xyz, 0.3, None, counts)
    got = run_gpu(dev, xyz, 0.3, None, counts)
    gr.assert_same(got, exp, "ragged tiles")
    check_consistent(got, n, counts)


def test_failure_statuses(dev):
    """a NaN or an inf among the valid points: status 2, ignored past the
    valid count; a grid finer than 2^20 cells along an axis: status 3; the
    clouds beside them are untouched"""
    n = 200
    rng = np.random.default_rng(12)
    xyz = rng.standard_normal((6, 3, n)).astype(F)
    feat = rng.standard_normal((6, 1, n)).astype(F)
    xyz[0, 2, 150] = np.nan
    xyz[1, 0, 150] = np.inf
    xyz[2, 1, 150] = np.nan   # past its valid count
    xyz[3, 1, 199] = -np.inf  # past its valid count
    xyz[4, 0, 0] = 3.0e5      # (3e5 - min) / 0.05 > 2^20
    counts = np.array([n, 151, 150, 199, n, n], np.int32)
    exp = gr.grid_subsample_batch(xyz, 0.05, feat, counts)
    assert exp["status"].tolist() == [2, 2, 0, 0, 3, 0]
    got = run_gpu(dev, xyz, 0.05, feat, counts)
    gr.assert_same(got, exp, "statuses")
    assert got["dims"][4, 0] > 1 << 20
    check_consistent(got, n, counts)
    # dims saturate
    two = np.array([[[0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]], F)
    for cell in (1e-30, 2.0 ** -20, 2.0 ** -19):
        exp = gr.grid_subsample_batch(two, cell)
        got = run_gpu(dev, two, cell)
        gr.assert_same(got, exp, cell)
    assert got["status"][0] == 0 and got["count"][0] == 2


def test_two_runs_give_the_same_bits(dev, shapes):
    xyz, feat, exp = shapes(3, 5000, 3, 0.2, seed=1)
    a = run_gpu(dev, xyz, 0.2, feat)
    b = run_gpu(dev, xyz, 0.2, feat)
    gr.assert_same(a, b, "rerun")
    gr.assert_same(a, exp, "restatement")
    check_consistent(a, 5000)


def test_largest_cloud(dev):
    """n = 262144 in one cloud (256 tiles), a dense cloud of about 4k cells"""
    n = 262144
    rng = np.random.default_rng(13)
    xyz = rng.random((1, 3, n)).astype(F)
    exp = gr.grid_subsample_batch(xyz, 1.0 / 16)
    got = run_gpu(dev, xyz, 1.0 / 16)
    gr.assert_same(got, exp, "large")
    assert got["count"][0] == 4096
    check_consistent(got, n)


def test_ops_and_numpy_mirror(dev):
    """ops.grid_subsample returns the C ABI's results under the documented
    keys, and io.grid_sub_sampling on one cloud equals the batched op"""
    from pcr_amd import io, ops
    rng = np.random.default_rng(14)
    n = 700
    xyz = rng.standard_normal((2, 3, n)).astype(F)
    feat = rng.standard_normal((2, 4, n)).astype(F)
    counts = np.array([n, 555], np.int32)
    ref = run_gpu(dev, xyz, 0.25, feat, counts)
    out = ops.grid_subsample(torch.from_numpy(xyz).to(dev), 0.25, torch.from_numpy(feat).to(dev),
                             torch.from_numpy(counts).to(dev))
    assert sorted(out) == sorted(["xyz", "features", "count", "cell_of", "cell_count", "origin",
                                  "dims", "status"])
    gr.assert_same({k: v.cpu().numpy() for k, v in out.items()}, ref, "ops")
    nofeat = ops.grid_subsample(torch.from_numpy(xyz).to(dev), 0.25)
    assert nofeat["features"] is None
    assert np.array_equal(nofeat["xyz"][0].cpu().numpy().view(np.uint32),
                          ref["xyz"][0].view(np.uint32))
    m = int(ref["count"][0])
    pts, fts = io.grid_sub_sampling(xyz[0].T, features=feat[0].T, grid_size=0.25)
    assert pts.shape == (m, 3) and fts.shape == (m, 4)
    assert np.array_equal(pts.view(np.uint32), ref["xyz"][0, :, :m].T.copy().view(np.uint32))
    assert np.array_equal(fts.view(np.uint32), ref["features"][0, :, :m].T.copy().view(np.uint32))
    only = io.grid_sub_sampling(xyz[0].T, grid_size=0.25)
    assert np.array_equal(only, pts)
    padded, cnt = io.pad_clouds([torch.from_numpy(xyz[0]).to(dev),
                                 torch.from_numpy(xyz[1, :, :555].copy()).to(dev)])
    rag = ops.grid_subsample(padded, 0.25, counts=cnt)
    assert np.array_equal(rag["xyz"].cpu().numpy().view(np.uint32), ref["xyz"].view(np.uint32))
