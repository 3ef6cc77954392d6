"""GPU: pcr_fpfh / ops.fpfh / registration.fpfh_pairs against the numpy
restatement (tests/fpfh_restate.py) with exact equality: fpfh, spfh and
nbr_count, floats compared as bit patterns.  The contract fixes every
operation and its order, so the tolerance is zero.  The neighbour lists come
from the numpy KNN, so only the new kernels are under test (ops.fpfh and the
end-to-end test feed the restatement with the oracle's KNN instead).

Every output buffer and the workspace are poisoned before each call (the C
ABI is called on buffers the test fills), so an element left unwritten fails.

Size thresholds of the implementation (csrc/fpfh.hip), each tested on both
sides:
  - 64 points per workgroup: n = 63, 64, 65; several tiles: n = 300, 1100
  - the SPFH stage takes slots in steps of 4 waves x 4 in flight: k = 1, 2,
    33, 64, 128
  - the FPFH stage stages 32 slots at a time, 8 rows in flight: k = 2, 33
    (one slot into the second chunk), 64, 128
  - n < k: the slots past n are never read (n = 1, 2, 65 with k = 2, 33, 128)
"""
import numpy as np
import pytest
import torch

import fpfh_restate as fr

pytestmark = pytest.mark.gpu
F = np.float32


def run_gpu(dev, xyz, normals, idx, dist, radius, want_spfh=True, want_count=True, stream=None,
            ws_short=0):
    """pcr_fpfh on poisoned outputs and a poisoned workspace -> fpfh, spfh,
    nbr_count as numpy (None for the outputs not asked for)"""
    from pcr_amd import _lib
    lib = _lib.load()
    b, _, n = xyz.shape
    k = idx.shape[1]
    tx = torch.from_numpy(np.ascontiguousarray(xyz, F)).to(dev)
    tn = torch.from_numpy(np.ascontiguousarray(normals, F)).to(dev)
    ti = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(dist, F)).to(dev)
    fp = torch.full((b, 33, n), float("nan"), dtype=torch.float32, device=dev)
    sp = torch.full((b, 33, n), float("nan"), dtype=torch.float32, device=dev) if want_spfh \
        else None
    cnt = torch.full((b, n), -7777, dtype=torch.int32, device=dev) if want_count else None
    need = lib.pcr_fpfh_workspace_size(b, n)
    ws = torch.full((max(256, need),), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def ptr(t):
        return None if t is None else t.data_ptr()
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.check(lib.pcr_fpfh(ptr(tx), ptr(tn), ptr(ti), ptr(td), b, n, k, float(radius), ptr(fp),
                            ptr(sp), ptr(cnt), ptr(ws), need - ws_short, st.cuda_stream), "fpfh")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (fp, sp, cnt))


def assert_same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("fpfh", "spfh", "nbr_count")):
        if g is not None:
            fr.assert_same_bits(g, e, (what, name))


@pytest.fixture(scope="module")
def expected():
    """(b, n, k, radius) -> (inputs, restatement), computed once"""
    cache = {}

    def get(b, n, k, radius):
        key = (b, n, k, radius)
        if key not in cache:
            inputs = fr.shape_inputs(b, n, k)
            cache[key] = (inputs, fr.fpfh(*inputs, radius))
        return cache[key]
    return get


@pytest.mark.parametrize("b,n,k,radius", fr.SHAPES)
def test_matches_the_restatement(dev, expected, b, n, k, radius):
    inputs, exp = expected(b, n, k, radius)
    got = run_gpu(dev, *inputs, radius)
    assert_same(got, exp, (b, n, k))
    assert np.isfinite(got[0]).all()


def test_radius_admits_nobody_or_everybody(dev, expected):
    b, n, k = 3, 300, 33
    inputs, _ = expected(b, n, k, 0.6)
    exp = fr.fpfh(*inputs, 1e-4)
    got = run_gpu(dev, *inputs, 1e-4)
    assert_same(got, exp, "nobody")
    assert not got[2].any() and not got[0].any() and not got[1].any()
    exp = fr.fpfh(*inputs, 10.0)
    got = run_gpu(dev, *inputs, 10.0)
    assert_same(got, exp, "everybody")
    assert (got[2] == k - 1).all()


def test_duplicates_and_salted_lists(dev):
    """a duplicated point, and lists salted with -1, n, INT_MAX, INT_MIN and
    NaN / negative / zero / infinite distances: skipped, never addresses"""
    xyz, nrm, idx, dist, radius = fr.salted_inputs()
    exp = fr.fpfh(xyz, nrm, idx, dist, radius)
    got = run_gpu(dev, xyz, nrm, idx, dist, radius)
    assert_same(got, exp, "salted")
    assert np.isfinite(got[0]).all()


def test_one_nan_normal_touches_itself_and_its_listers(dev, expected):
    (xyz, nrm, idx, dist), clean = expected(1, 300, 33, 0.45)
    bad = nrm.copy()
    bad[0, 1, 17] = np.nan
    exp = fr.fpfh(xyz, bad, idx, dist, 0.45)
    got = run_gpu(dev, xyz, bad, idx, dist, 0.45)
    assert_same(got, exp, "nan normal")
    assert np.isfinite(got[0]).all()
    listing = fr.listers(idx[0], dist[0], 300, 0.45, 17)
    changed = (got[1][0].view(np.uint32) != clean[1][0].view(np.uint32)).any(axis=0)
    assert changed[17] and not (changed & ~listing).any()
    ring = listing.copy()
    for p in np.nonzero(listing)[0]:
        ring |= fr.listers(idx[0], dist[0], 300, 0.45, p)
    changed = (got[0][0].view(np.uint32) != clean[0][0].view(np.uint32)).any(axis=0)
    assert changed[17] and not (changed & ~ring).any() and not ring.all()


def test_optional_outputs_stream_and_rerun(dev, expected):
    """spfh and nbr_count NULL; a non-default stream; two runs, the same bits"""
    inputs, exp = expected(3, 300, 128, 0.6)
    only = run_gpu(dev, *inputs, 0.6, want_spfh=False, want_count=False)
    assert only[1] is None and only[2] is None
    assert_same(only, exp, "fpfh alone")
    side = torch.cuda.Stream(device=dev)
    a = run_gpu(dev, *inputs, 0.6, stream=side)
    b = run_gpu(dev, *inputs, 0.6, stream=side)
    assert_same(a, exp, "side stream")
    assert_same(b, a, "rerun")


def test_short_workspace_is_refused(dev, expected):
    inputs, _ = expected(1, 64, 33, 0.6)
    with pytest.raises(RuntimeError, match="workspace too small"):
        run_gpu(dev, *inputs, 0.6, ws_short=1)


def test_ops_fpfh_past_the_knn_4096_path(dev):
    """ops.fpfh at n = 4100, k = 16 (its KNN included) against the restatement
    fed with the oracle's KNN; return_spfh / return_counts order"""
    import oracle
    from pcr_amd import ops
    n, k, radius = 4100, 16, 0.1
    xyz, nrm = (a[None] for a in fr.surface(n, seed=41))
    d1, _, i1, _ = oracle.knn_forward(xyz, xyz, k)
    exp = fr.fpfh(xyz, nrm, i1, d1, radius)
    assert 2 <= exp[2].min() and exp[2].max() == k - 1
    tx, tn = torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev)
    got = ops.fpfh(tx, tn, radius, k=k, return_spfh=True, return_counts=True)
    assert_same(tuple(t.cpu().numpy() for t in got), exp, "ops.fpfh")
    alone = ops.fpfh(tx, tn, radius, k=k)
    fr.assert_same_bits(alone.cpu().numpy(), exp[0], "ops.fpfh alone")
    fp, cnt = ops.fpfh(tx, tn, radius, k=k, return_counts=True)
    fr.assert_same_bits(cnt.cpu().numpy(), exp[2], "counts")


# ------------------------------------------------------------- end to end
def rotation_error(gt, est):
    """The angle of Rgt^T Rest in degrees, as 2 asin(|Rgt - Rest|_F / (2
    sqrt 2)): the angle RE_TE_one_pair's acos((tr - 1) / 2) measures, in a form
    that resolves angles below 1e-6 degrees (the acos form reads 0 or 1.7e-6
    there: 1 - cos of the angle is below the spacing of doubles at 1)."""
    d = np.linalg.norm(np.asarray(gt)[:3, :3] - np.asarray(est)[:3, :3])
    return float(np.degrees(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0))))))


@pytest.fixture(scope="module")
def pair():
    """the surface (n = 512, seed 11) and its moved, permuted copy; their
    restatement features on the oracle's KNN (k = 32, r = 0.3); the numpy
    mutual nearest neighbours of those"""
    import oracle
    n, k, radius = 512, 32, 0.3
    xyz, nrm = fr.surface(n, seed=11)
    x2, n2, perm, gt = fr.moved_copy(xyz, nrm, seed=12)
    d1, _, i1, _ = oracle.knn_forward(xyz[None], xyz[None], k)
    d2, _, i2, _ = oracle.knn_forward(x2[None], x2[None], k)
    fa = fr.fpfh(xyz[None], nrm[None], i1, d1, radius)[0]
    fb = fr.fpfh(x2[None], n2[None], i2, d2, radius)[0]
    m1, m2 = fr.mutual_nn(fa[0], fb[0])
    idx1, idx2 = np.full((1, n), -1, np.int32), np.full((1, n), -1, np.int32)
    idx1[0, :len(m1)], idx2[0, :len(m1)] = m1, m2
    return dict(xyz=xyz[None], nrm=nrm[None], x2=x2[None], n2=n2[None], perm=perm, gt=gt, fa=fa,
                fb=fb, idx1=idx1, idx2=idx2, count=np.array([len(m1)], np.int32), k=k,
                radius=radius)


@pytest.mark.parametrize("solver", ["ransac", "fgr"])
def test_fpfh_pairs_end_to_end(dev, pair, solver):
    """registration.fpfh_pairs on the moved, permuted copy: the GPU features
    are the restatement's bits, the mutual count and pairs the numpy matcher's
    (510 of the 512 points, every one its own copy; the other two tie within
    the fp32 rounding of the feature distance), and the rotation and
    translation errors stay below 10 x what the CPU chain (restatement
    features, numpy mutual-NN, rigid_restate / fgr_restate) reaches on the
    same input.  Measured with the CPU chain: ransac 5.2e-08 degrees and
    1.5e-09, fgr 4.9e-08 degrees and 1.7e-09 (the fp32 rounding of the moved
    copy)."""
    import fgr_restate
    import rigid_restate
    from pcr_amd import registration
    p = pair
    if solver == "ransac":
        cpu = rigid_restate.ransac(p["xyz"], p["x2"], p["idx1"], p["idx2"], p["count"], 1000, 0.08,
                                   0.9, 2, 0)
    else:
        cpu = fgr_restate.fgr(p["xyz"], p["x2"], p["idx1"], p["idx2"], p["count"])
    assert cpu["status"][0] == 0
    cpu_rre = rotation_error(p["gt"], cpu["transform"][0])
    cpu_rte = float(np.linalg.norm(p["gt"][:3, 3] - cpu["transform"][0][:3, 3]))
    print("%s CPU chain: rre %.3g degrees, rte %.3g" % (solver, cpu_rre, cpu_rte))
    assert 0 < cpu_rre < 1e-5 and 0 < cpu_rte < 1e-7

    def T(a):
        return torch.from_numpy(a).to(dev)
    out = registration.fpfh_pairs(T(p["xyz"]), T(p["nrm"]), T(p["x2"]), T(p["n2"]), p["radius"],
                                  k=p["k"], solver=solver)
    fr.assert_same_bits(out["feat1"].cpu().numpy(), p["fa"], "feat1")
    fr.assert_same_bits(out["feat2"].cpu().numpy(), p["fb"], "feat2")
    count = int(out["count"][0])
    assert count == int(p["count"][0])
    i1, i2 = out["idx1"][0, :count].cpu().numpy(), out["idx2"][0, :count].cpu().numpy()
    assert np.array_equal(i1, p["idx1"][0, :count]) and np.array_equal(i2, p["idx2"][0, :count])
    assert int((p["perm"][i2] == i1).sum()) >= 0.95 * 512
    assert int(out["reg_status"][0]) == 0
    est = out["transform"][0].cpu().numpy()
    rre = rotation_error(p["gt"], est)
    rte = float(np.linalg.norm(p["gt"][:3, 3] - est[:3, 3]))
    print("%s GPU: rre %.3g degrees, rte %.3g" % (solver, rre, rte))
    assert rre <= 10 * cpu_rre and rte <= 10 * cpu_rte
