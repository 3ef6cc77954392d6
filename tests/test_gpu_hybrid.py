"""GPU: pcr_hybrid_search / ops.hybrid_search / ops.fpfh(search="grid") /
registration.fpfh_pairs(search="grid") against the numpy restatement
(tests/hybrid_restate.py: brute force over all pairs, no cells) with exact
equality: distances as bit patterns, indices, counts.  The contract fixes the
result for every input, so the tolerance is zero.

Every output buffer and the workspace are poisoned before each call (the C
ABI is called on buffers the test fills), so an element left unwritten fails.
Each input's purpose is asserted on the restatement (hr.assert_reaches), not
on the code under test.

Thresholds of the implementation (csrc/hybrid_search.hip) and the inputs on
both sides of them:
  - 32 queries per workgroup, a wave per query: n = 1, 2, 63, 65, 129
  - the sort holds 64 or 128 keys: k = 1, 7, 16, 100, 128, and k > n
  - within <= k (sorted as found), within > k (radix selection from the
    wave's buffer): "both"; within > PCR_HYBRID_WAVE_CAP (selection by sweeps
    over the cells): "overflow"
  - one cell (no finite extent, or a radius above the cloud) and the bounded
    grid (a radius far below the extent): "huge", "overflow", "tiny_radius"
"""
import numpy as np
import pytest
import torch

import hybrid_restate as hr

pytestmark = pytest.mark.gpu
F = np.float32


def run_gpu(dev, xyz, radius, k, counts=None, want_within=True):
    """pcr_hybrid_search on poisoned outputs and a poisoned workspace -> dist,
    idx, nbr_count, within as numpy (within None when not asked for)"""
    from pcr_amd import _lib
    lib = _lib.load()
    b, _, n = xyz.shape
    tx = torch.from_numpy(np.ascontiguousarray(xyz, F)).to(dev)
    tc = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(dev)
    dist = torch.full((b, k, n), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((b, k, n), -7777, dtype=torch.int32, device=dev)
    cnt = torch.full((b, n), -7777, dtype=torch.int32, device=dev)
    win = torch.full((b, n), -7777, dtype=torch.int32, device=dev) if want_within else None
    need = lib.pcr_hybrid_search_workspace_size(b, n)
    ws = torch.full((max(256, need),), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def ptr(t):
        return None if t is None else t.data_ptr()
    status = lib.pcr_hybrid_search(ptr(tx), ptr(tc), b, n, k, float(radius), ptr(dist), ptr(idx),
                                   ptr(cnt), ptr(win), ptr(ws), need,
                                   torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib.pcr_last_error()  # PCR_OK
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (dist, idx, cnt, win))


def check_case(dev, name):
    hr.assert_reaches(name)
    xyz, radius, ks, counts = hr.cases()[name]
    for k in ks:
        got = run_gpu(dev, xyz, radius, k, counts)
        hr.assert_same(got, hr.expected(name, k), (name, k))


@pytest.mark.parametrize("n", [1, 2, 63, 65, 129])
def test_sizes(dev, n):
    """b = 3 with a different cloud in each slot; k = 1, 7 and 128 (> n up to 65)"""
    check_case(dev, "size_%d" % n)


def test_both_branches_in_one_cloud(dev):
    """300 points, k = 16: queries with fewer than k, exactly k and more than k
    within the radius"""
    check_case(dev, "both")


def test_more_within_the_radius_than_a_wave_buffers(dev):
    """n = 1500 in one cell, every query has all 1500 within its radius, above
    PCR_HYBRID_WAVE_CAP: k = 128 and k = 5 select by sweeps over the cell"""
    check_case(dev, "overflow")


@pytest.mark.parametrize("name", ["lattice", "lattice_shifted", "lattice_inside",
                                  "lattice_outside"])
def test_cell_edges_and_ties(dev, name):
    """a 6 x 6 x 6 lattice at spacing = radius = 0.25 exactly (neighbours at
    d == r2, on cell faces), shifted, and one ulp inside / outside; k = 4 cuts
    inside six equal distances"""
    check_case(dev, name)


@pytest.mark.parametrize("name", ["tiny_radius", "far_from_origin"])
def test_sparse_and_fine(dev, name):
    check_case(dev, name)


def test_duplicates(dev):
    """200 copies of one point and 100 others, k = 128: a copy with index >=
    128 lists copies 0 .. 127 and not itself"""
    check_case(dev, "duplicates")


@pytest.mark.parametrize("name", ["ragged_nan", "ragged_copies"])
def test_ragged(dev, name):
    """counts = [130, 0, 1, 77] of n = 130; the padding holds NaN, or copies of
    valid points that would be neighbours"""
    check_case(dev, name)
    xyz, radius, ks, counts = hr.cases()[name]
    dist, idx, cnt, within = run_gpu(dev, xyz, radius, ks[-1], counts)
    for q, m in enumerate(counts):
        assert (idx[q, :, m:] == -1).all() and np.isposinf(dist[q, :, m:]).all()
        assert not cnt[q, m:].any() and not within[q, m:].any()
        assert idx[q].max() < max(int(m), 1)


@pytest.mark.parametrize("name", ["non_finite", "huge"])
def test_non_finite_and_huge(dev, name):
    """a NaN point, a +inf point and a -inf coordinate among valid points;
    coordinates of +-3e38 beside an ordinary cluster: PCR_OK (run_gpu asserts
    it) and the restatement's rows"""
    check_case(dev, name)


def test_within_is_optional(dev):
    xyz, radius, ks, counts = hr.cases()["both"]
    got = run_gpu(dev, xyz, radius, 16, want_within=False)
    assert got[3] is None
    hr.assert_same(got, hr.expected("both", 16), "no within")


def test_determinism_and_permutation(dev):
    """the same call twice gives the same bits; a permuted cloud gives rows
    that are the permutation's image: distances equal, indices mapped.  (Ties
    between different neighbours would reorder under a permutation, so this
    cloud is checked on the restatement to have none inside a row.)"""
    xyz, radius, _, _ = hr.cases()["both"]
    k = 16
    more = hr.search(xyz, radius, k + 1)  # one more slot: no tie across the cut either
    d = more[0][0]
    filled = np.arange(k + 1)[:, None] < more[2][0][None, :]
    assert not ((d[1:] == d[:-1]) & filled[1:]).any()
    a = run_gpu(dev, xyz, radius, k)
    b = run_gpu(dev, xyz, radius, k)
    hr.assert_same(a, b, "twice")
    perm = np.random.default_rng(5).permutation(xyz.shape[2])  # new point s is old perm[s]
    inv = np.argsort(perm)
    got = run_gpu(dev, xyz[:, :, perm], radius, k)
    hr.assert_same_bits(got[0], a[0][:, :, perm], "dist")
    old = a[1][:, :, perm]
    mapped = np.where(old >= 0, inv[np.maximum(old, 0)], -1).astype(np.int32)
    hr.assert_same_bits(got[1], mapped, "idx")
    hr.assert_same_bits(got[2], a[2][:, perm], "count")
    hr.assert_same_bits(got[3], a[3][:, perm], "within")


@pytest.fixture(scope="module")
def surfaces():
    """3 x 257 finite surface clouds with normals (tests/fpfh_restate.py)"""
    import fpfh_restate as fr
    per = [fr.surface(257, seed=60 + q) for q in range(3)]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])


@pytest.mark.parametrize("k", [32, 100])
def test_against_the_existing_knn(dev, surfaces, k):
    """hybrid rows equal knn_forward_cuda(xyz, xyz, k) in every slot below
    nbr_count; ops.fpfh(search="grid") is ops.fpfh(search="knn") bit for bit"""
    from pcr_amd import ops
    xyz, nrm = surfaces
    radius = {32: 0.5, 100: 1.0}[k]
    exp = hr.search(xyz, radius, k)
    # the radius cuts some rows and max_nn others
    assert (exp[3] < k).any() and (exp[3] > k).any() and (exp[2] >= 2).all()
    tx, tn = torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev)
    dist, idx, cnt, within = (t.cpu().numpy() for t in
                              ops.hybrid_search(tx, radius, k, return_within=True))
    hr.assert_same((dist, idx, cnt, within), exp, "ops.hybrid_search")
    three = ops.hybrid_search(tx, radius, k)
    assert len(three) == 3
    kd, _, ki, _ = (t.cpu().numpy() for t in ops.knn_forward_cuda(tx, tx, k))
    filled = np.arange(k)[None, :, None] < cnt[:, None, :]
    assert np.array_equal(idx[filled], ki[filled])
    assert np.array_equal(dist[filled].view(np.uint32), kd[filled].view(np.uint32))
    grid = ops.fpfh(tx, tn, radius, k=k, search="grid", return_spfh=True, return_counts=True)
    knn = ops.fpfh(tx, tn, radius, k=k, search="knn", return_spfh=True, return_counts=True)
    plain = ops.fpfh(tx, tn, radius, k=k)
    for g, e, what in zip(grid, knn, ("fpfh", "spfh", "counts")):
        hr.assert_same_bits(g.cpu().numpy(), e.cpu().numpy(), what)
    hr.assert_same_bits(plain.cpu().numpy(), knn[0].cpu().numpy(), "the default is knn")
    assert np.isfinite(grid[0].cpu().numpy()).all() and grid[0].abs().sum() > 0


def test_ragged_fpfh(dev):
    """two clouds of different size padded together with counts: per cloud
    bit for bit ops.fpfh of that cloud alone, and zero at or past the count"""
    import fpfh_restate as fr
    from pcr_amd import ops
    sizes, n, radius, k = (200, 131), 200, 0.3, 32
    clouds = [fr.surface(m, seed=70 + q) for q, m in enumerate(sizes)]
    xyz, nrm = np.zeros((2, 3, n), F), np.zeros((2, 3, n), F)
    for q, (p, nn) in enumerate(clouds):
        xyz[q, :, :sizes[q]], nrm[q, :, :sizes[q]] = p, nn
        # padding that would be neighbours if it were read
        xyz[q, :, sizes[q]:] = p[:, :n - sizes[q]]
        nrm[q, :, sizes[q]:] = nn[:, :n - sizes[q]]
    counts = torch.tensor(sizes, dtype=torch.int32, device=dev)
    got = ops.fpfh(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), radius, k=k,
                   search="grid", counts=counts).cpu().numpy()
    for q, (p, nn) in enumerate(clouds):
        alone = ops.fpfh(torch.from_numpy(p[None]).to(dev), torch.from_numpy(nn[None]).to(dev),
                         radius, k=k).cpu().numpy()
        assert np.abs(alone).sum() > 0
        hr.assert_same_bits(got[q, :, :sizes[q]], alone[0], "cloud %d" % q)
        assert not got[q, :, sizes[q]:].any()


def test_fpfh_pairs_with_the_grid_search(dev):
    """registration.fpfh_pairs on test_gpu_fpfh.py's end-to-end case (the
    512-point surface and its rotated, permuted copy): the rotation error with
    search="grid" does not exceed that of search="knn" in the same run"""
    import fpfh_restate as fr
    from pcr_amd import registration
    n, k, radius = 512, 32, 0.3

    def rotation_error(gt, est):
        """the angle of Rgt^T Rest in degrees, as test_gpu_fpfh.py measures it"""
        d = np.linalg.norm(np.asarray(gt)[:3, :3] - np.asarray(est)[:3, :3])
        return float(np.degrees(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0))))))
    xyz, nrm = fr.surface(n, seed=11)
    x2, n2, perm, gt = fr.moved_copy(xyz, nrm, seed=12)

    def T(a):
        return torch.from_numpy(a[None]).to(dev)
    out = {s: registration.fpfh_pairs(T(xyz), T(nrm), T(x2), T(n2), radius, k=k, search=s)
           for s in ("knn", "grid")}
    rre = {s: rotation_error(gt, o["transform"][0].cpu().numpy()) for s, o in out.items()}
    print("rotation error: knn %.3g degrees, grid %.3g degrees" % (rre["knn"], rre["grid"]))
    assert int(out["grid"]["reg_status"][0]) == 0
    hr.assert_same_bits(out["grid"]["feat1"].cpu().numpy(), out["knn"]["feat1"].cpu().numpy(), "f1")
    hr.assert_same_bits(out["grid"]["feat2"].cpu().numpy(), out["knn"]["feat2"].cpu().numpy(), "f2")
    assert rre["grid"] <= rre["knn"]


def test_invalid_arguments(dev):
    from pcr_amd import ops
    x = torch.zeros((2, 3, 8), device=dev)
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1e20):
        with pytest.raises(RuntimeError, match="radius"):
            ops.hybrid_search(x, radius, 4)
    for k in (0, 129):
        with pytest.raises(RuntimeError, match="k must be"):
            ops.hybrid_search(x, 0.1, k)
    counts = torch.full((2,), 8, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="counts needs search='grid'"):
        ops.fpfh(x, x, 0.1, k=4, counts=counts)
    with pytest.raises(RuntimeError, match="search must be"):
        ops.fpfh(x, x, 0.1, k=4, search="tree")
    with pytest.raises(RuntimeError, match="expected counts"):
        ops.hybrid_search(x, 0.1, 4, counts=torch.zeros((3,), dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="must be an int tensor"):
        ops.hybrid_search(x, 0.1, 4, counts=torch.zeros((2,), device=dev))
