"""GPU: pcr_icp_point_to_plane (csrc/icp_plane.hip) through ops.icp and
pcr_amd.registration against the numpy restatement of its contract
(tests/icp_plane_restate.py).

Synthetic pairs (icp_plane_restate.make_pair): source points on an ellipsoid
with semi-axes 1 / 0.8 / 0.6, the target a permuted superset or subset moved
by R a + t with the moved analytic normals, rounded to fp32; max_dist = 0.2.
Bounds:
  exact     corr, num_corr, iterations, status and fitness equal the
            restatement: the decisions are the same fp32 operations on both
            sides, under the asserted input condition that no convergence test
            lies within 1e-9 of its tolerance;
  rmse      1e-12 relative: fp64 sums of at most a few thousand non-negative
            terms in two orders;
  transform 10 x the largest difference between the gcc run of the headers and
            the restatement that tests/test_icp_plane_cpu.py measured over its
            cases (these shapes among them): 3.747e-16, on the 6 x 6 pair.
            The kernel differs from the gcc run in the order of the sums only;
  recovery  1e-5 against the ground truth where every source has its
            counterpart: the fp32 rounding of the targets.
The workgroup's tile is 1024 source points (n1100 takes two) and the LDS chunk
8192 targets (n100_9000 takes two, n1030_8200 two of each)."""
import functools

import numpy as np
import pytest
import torch

import icp_plane_restate as pr
import icp_restate as ir

pytestmark = pytest.mark.gpu

DEFAULTS = dict(max_dist=0.2, max_iters=200, rel_fitness=1e-6, rel_rmse=1e-6)
CPU_MEASURED = 3.747e-16  # gcc versus numpy, the largest transform difference
TBOUND = 10 * CPU_MEASURED
assert TBOUND <= 1e-6


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


# name -> (seed, p, n1, n2, make_pair keywords, icp keywords, recovers the ground truth)
CASES = {
    "n6": (209, 1, 6, 6, {}, {}, True),  # M exactly at the threshold
    "n5_8": (202, 1, 5, 8, {}, {}, False),  # status 1
    "n64": (203, 2, 64, 64, {}, {}, True),
    "n1100_1024": (204, 1, 1100, 1024, {}, {}, False),  # 76 sources have no counterpart
    "n100_9000": (205, 1, 100, 9000, {}, {}, True),
    "n1030_8200": (206, 1, 1030, 8200, {}, dict(max_iters=1), False),
    "init": (207, 2, 128, 128, dict(degrees=120.0, tnorm=0.3), {}, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    seed, p, n1, n2, mk, kw, _ = CASES[name]
    x1, x2, nr, gt = pr.make_batch(seed, p, n1, n2, **mk)
    init = None
    if name == "init":
        rng = np.random.default_rng(seed)
        init = np.stack([g @ ir.motion(rng, 3.0, 0.02) for g in gt])
    args = dict(DEFAULTS, **kw)
    exp = pr.icp(x1, x2, nr, init, **args)
    return x1, x2, nr, gt, init, args, exp


def run(dev, x1, x2, nr, init=None, counts1=None, counts2=None, **kw):
    from pcr_amd import ops
    out = ops.icp(T(x1, dev), T(x2, dev), None if init is None else T(init, dev),
                  counts1=None if counts1 is None else T(np.asarray(counts1, np.int32), dev),
                  counts2=None if counts2 is None else T(np.asarray(counts2, np.int32), dev),
                  estimation="point_to_plane", normals2=T(nr, dev), **kw)
    torch.cuda.synchronize()
    return dict(zip(ir.KEYS, (N(o) for o in out)))


def assert_matches(got, exp, name=""):
    for k in ("status", "iterations", "num_corr", "corr"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (name, k)
    assert np.array_equal(got["fitness"], exp["fitness"]), name
    rel = np.abs(got["rmse"] - exp["rmse"]) / np.maximum(exp["rmse"], 1e-300)
    dt = np.abs(got["transform"] - exp["transform"]).max()
    print("%s: iterations %s, rmse rel %.3g, transform %.3g" % (
        name, got["iterations"].tolist(), rel.max(), dt))
    assert rel.max() <= 1e-12, name
    assert got["transform"].dtype == np.float64 and dt <= TBOUND, name
    bottom = np.tile([0.0, 0.0, 0.0, 1.0], (len(exp["status"]), 1))
    assert np.array_equal(got["transform"][:, 3], bottom), name


def assert_self_consistent(x1, x2, got, max_dist):
    """Evaluate at the returned transform gives the returned corr / num_corr / rmse"""
    for q in range(len(x1)):
        ev = ir.evaluate(got["transform"][q, :3, :3], got["transform"][q, :3, 3],
                         np.ascontiguousarray(x1[q].T), np.ascontiguousarray(x2[q].T), max_dist)
        assert np.array_equal(ev["corr"], got["corr"][q]), q
        assert ev["num_corr"] == got["num_corr"][q] == (got["corr"][q] >= 0).sum(), q
        assert ev["fitness"] == got["fitness"][q], q
        assert abs(ev["rmse"] - got["rmse"][q]) <= 1e-12 * max(ev["rmse"], 1e-300), q


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(dev, name):
    x1, x2, nr, gt, init, args, exp = case(name)
    assert exp["conv_margin"] > 1e-9  # the input condition of the exact comparison
    got = run(dev, x1, x2, nr, init, **args)
    assert_matches(got, exp, name)
    assert_self_consistent(x1, x2, got, args["max_dist"])
    n1 = x1.shape[2]
    if name not in ("n5_8", "n1030_8200"):
        assert (exp["status"] == 0).all() and (exp["iterations"] >= 1).all()
    if CASES[name][6]:
        err = np.abs(got["transform"] - gt).max()
        print("%s: recovery %.3g" % (name, err))
        assert err <= 1e-5
        assert (got["num_corr"] == n1).all()
    if name == "n6":
        assert got["num_corr"].tolist() == [6]
    if name == "n5_8":
        assert got["status"].tolist() == [1] and got["iterations"].tolist() == [0]
        assert got["num_corr"].tolist() == [5]
        assert np.array_equal(got["transform"][0], np.eye(4))
    if name == "n1100_1024":
        assert (got["num_corr"] >= 1024).all()
    if name == "n100_9000":
        assert (got["corr"] >= 8192).any()  # a normal gathered from beyond the first chunk
    if name == "n1030_8200":
        assert exp["status"].tolist() == [2] and exp["iterations"].tolist() == [1]
    if name == "init":
        # from the identity the 120 degree pair does not get there
        cold = run(dev, x1, x2, nr, None, **args)
        assert np.abs(cold["transform"] - gt).max() > 0.1


def test_planar_target_is_status_3_and_keeps_the_init(dev):
    x1, x2, nr = pr.planar_pair(21)
    exp = pr.icp_pair(x1, x2, nr, None, **DEFAULTS)
    assert (exp["status"], exp["iterations"]) == (3, 0)
    got = run(dev, x1[None], x2[None], nr[None], **DEFAULTS)
    assert got["status"].tolist() == [3] and got["iterations"].tolist() == [0]
    assert got["transform"][0].tobytes() == np.eye(4).tobytes()
    assert np.array_equal(got["corr"][0], exp["corr"]) and got["num_corr"][0] == exp["num_corr"]
    init = ir.motion(np.random.default_rng(3), 0.5, 0.01)[None]
    kept = run(dev, x1[None], x2[None], nr[None], init, **DEFAULTS)
    assert kept["status"].tolist() == [3]
    assert kept["transform"][0].tobytes() == init[0].tobytes()
    assert_self_consistent(x1[None], x2[None], kept, DEFAULTS["max_dist"])


def test_nan_normal_is_status_3_and_the_batch_goes_on(dev):
    x1, x2, nr, gt, _, args, exp = case("n64")
    b1, b2, bn, _ = pr.make_batch(211, 1, 64, 64, degrees=0.1, tnorm=0.001)
    bn = bn.copy()
    bn[0, :, 5] = np.nan
    bexp = pr.icp_pair(b1[0], b2[0], bn[0], None, **args)
    assert bexp["status"] == 3 and 5 in bexp["corr"]
    m1, m2, mn = (np.concatenate((a[:1], b, a[1:])) for a, b in ((x1, b1), (x2, b2), (nr, bn)))
    got = run(dev, m1, m2, mn, **args)
    clean = run(dev, x1, x2, nr, **args)
    assert got["status"].tolist() == [0, 3, 0]
    assert got["iterations"][1] == bexp["iterations"]
    assert np.array_equal(got["corr"][1], bexp["corr"])
    assert np.isfinite(got["transform"]).all()
    assert np.abs(got["transform"][1] - bexp["transform"]).max() <= TBOUND
    for k in ir.KEYS:
        assert got[k][[0, 2]].tobytes() == clean[k].tobytes(), k
    assert_self_consistent(m1, m2, got, args["max_dist"])


def test_limits_and_pure_evaluation(dev):
    x1, x2, nr, gt, _, args, exp = case("n64")
    for iters, st in ((1, 2), (0, 2)):
        kw = dict(args, max_iters=iters)
        e = pr.icp(x1, x2, nr, None, **kw)
        got = run(dev, x1, x2, nr, **kw)
        assert_matches(got, e, "max_iters=%d" % iters)
        assert got["status"].tolist() == [st, st] and got["iterations"].tolist() == [iters] * 2
        assert_self_consistent(x1, x2, got, args["max_dist"])
    assert np.array_equal(got["transform"], np.tile(np.eye(4), (2, 1, 1)))


def test_sampling_case_against_point_to_point(dev):
    """Two independent samplings of one ellipsoid (400 x 4000): the plane step
    ends at a tenth of point-to-point's transform error or less, in fewer
    iterations, within 1e-3 of the ground truth."""
    from pcr_amd import ops
    x1, x2, nr, gt = pr.sampling_pair(31)
    exp = pr.icp_pair(x1, x2, nr, None, **DEFAULTS)
    assert exp["conv_margin"] > 1e-9
    got = run(dev, x1[None], x2[None], nr[None], **DEFAULTS)
    assert_matches(got, {k: np.asarray(exp[k])[None] for k in ir.KEYS}, "sampling")
    point = dict(zip(ir.KEYS, (N(o) for o in ops.icp(T(x1[None], dev), T(x2[None], dev),
                                                     **DEFAULTS))))
    e_plane = pr.transform_error(got["transform"][0], gt)
    e_point = pr.transform_error(point["transform"][0], gt)
    print("sampling: plane %d iterations, error %.3e; point %d iterations, error %.3e"
          % (got["iterations"][0], e_plane, point["iterations"][0], e_point))
    assert got["status"][0] == 0 and point["status"][0] == 0
    assert e_plane <= e_point / 10
    assert got["iterations"][0] < point["iterations"][0]
    assert e_plane <= 1e-3


def test_deterministic_and_batch_independent(dev):
    for name in ("n64", "n1100_1024", "n100_9000"):
        x1, x2, nr, gt, _, args, exp = case(name)
        one, two = run(dev, x1, x2, nr, **args), run(dev, x1, x2, nr, **args)
        for k in ir.KEYS:
            assert one[k].tobytes() == two[k].tobytes(), (name, k)
    x1, x2, nr, gt, _, args, exp = case("n64")
    one = run(dev, x1, x2, nr, **args)
    for q in range(len(x1)):
        alone = run(dev, x1[q:q + 1], x2[q:q + 1], nr[q:q + 1], **args)
        for k in ir.KEYS:
            assert alone[k][0].tobytes() == one[k][q].tobytes(), (q, k)


# ----------------------------------------------------------------- ragged
def padded(rng, a, n, how):
    """[3, v] -> [3, n] with NaN pads or pads copied from the cloud"""
    out = np.full((3, n), np.nan, np.float32)
    v = a.shape[1]
    out[:, :v] = a
    if how == "copy" and v:
        out[:, v:] = a[:, rng.integers(0, v, n - v)]
    return out


def ragged_batch(seed, n1, n2, counts):
    """pairs of the given (v1, v2), padded to the strides n1 / n2: NaN pads in
    the even pairs, copied points and normals in the odd ones"""
    rng = np.random.default_rng(seed)
    trimmed, b1, b2, bn = [], [], [], []
    for q, (v1, v2) in enumerate(counts):
        x1, x2, nr, _ = pr.make_pair(rng, max(v1, 1), max(v2, 1))
        x1, x2, nr = x1[:, :v1], x2[:, :v2], nr[:, :v2]
        trimmed.append((x1, x2, nr))
        how = "copy" if q % 2 else "nan"
        b1.append(padded(rng, x1, n1, how))
        b2.append(padded(rng, x2, n2, how))
        bn.append(padded(rng, nr, n2, how))
    return trimmed, np.stack(b1), np.stack(b2), np.stack(bn)


@pytest.mark.parametrize("n1,n2,counts", [
    (64, 64, ((0, 50), (40, 0), (5, 64), (64, 64), (33, 47))),
    (1100, 8200, ((1030, 300), (200, 8200))),
], ids=["small", "chunked"])
def test_ragged_pairs_are_the_trimmed_pairs_in_bits(dev, n1, n2, counts):
    trimmed, b1, b2, bn = ragged_batch(220 + n1, n1, n2, counts)
    init = np.stack([ir.motion(np.random.default_rng(q), 0.5, 0.005) for q in range(len(counts))])
    c1, c2 = [c[0] for c in counts], [c[1] for c in counts]
    got = run(dev, b1, b2, bn, init, counts1=c1, counts2=c2, **DEFAULTS)
    for q, (v1, v2) in enumerate(counts):
        x1, x2, nr = trimmed[q]
        assert (got["corr"][q, v1:] == -1).all(), q
        if v1 == 0:
            assert got["transform"][q].tobytes() == init[q].tobytes()
            assert (got["status"][q], got["iterations"][q], got["num_corr"][q]) == (1, 0, 0)
            assert got["fitness"][q] == 0.0 and got["rmse"][q] == 0.0
            continue
        if v2 == 0:
            assert (got["status"][q], got["iterations"][q], got["num_corr"][q]) == (1, 0, 0)
            assert got["transform"][q].tobytes() == init[q].tobytes()
            assert (got["corr"][q] == -1).all() and got["fitness"][q] == 0.0
            zero = run(dev, b1, b2, bn, init, counts1=c1, counts2=c2,
                       **dict(DEFAULTS, max_iters=0))
            assert zero["status"][q] == 2
            continue
        alone = run(dev, x1[None], x2[None], nr[None], init[q:q + 1], **DEFAULTS)
        for k in ir.KEYS:
            a = alone[k][0]
            g = got[k][q][:v1] if k == "corr" else got[k][q]
            assert g.tobytes() == a.tobytes(), (q, k)
        if v1 == 5:
            assert got["status"][q] == 1 and got["num_corr"][q] == 5
        else:
            assert got["status"][q] in (0, 2) and got["iterations"][q] >= 1
    # counts on one side only, and counts beyond the stride are clamped
    full = run(dev, b1[3:4], b2[3:4], bn[3:4], init[3:4], **DEFAULTS) if n1 == 64 else None
    if full is not None:
        over = run(dev, b1[3:4], b2[3:4], bn[3:4], init[3:4], counts1=[1000], **DEFAULTS)
        for k in ir.KEYS:
            assert over[k].tobytes() == full[k].tobytes(), k


# ----------------------------------------------------------- registration
PLANE = dict(estimation="point_to_plane")


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    else:
        assert N(a).tobytes() == N(b).tobytes(), what


def test_scan_and_fpfh_pairs_refine_along_the_target_normals(dev):
    """scan_pairs and fpfh_pairs fill normals2 from the target normals they
    hold: status 0, the alignment no worse than the point-to-point
    refinement's on the same input, and estimation="point_to_point" is the
    call without the keyword, in bits."""
    import ragged_restate as rr
    from pcr_amd import ops, registration as reg
    pairs = [rr.scan_pair(900 + q, n1, n2) for q, (n1, n2) in enumerate(((2000, 2600),
                                                                         (2500, 2100)))]
    s1 = [T(a, dev) for a, _, _ in pairs]
    s2 = [T(b, dev) for _, b, _ in pairs]
    gt = T(np.stack([g for _, _, g in pairs]), dev)
    cell = 0.1
    point = reg.scan_pairs(s1, s2, cell, icp={})
    named = reg.scan_pairs(s1, s2, cell, icp=dict(estimation="point_to_point"))
    plane = reg.scan_pairs(s1, s2, cell, icp=PLANE)
    torch.cuda.synchronize()
    assert set(named) == set(point) == set(plane)
    for k in point:
        same(named[k], point[k], k)
        if not k.startswith("icp_"):
            same(plane[k], point[k], k)
    assert (N(plane["reg_status"]) == 0).all() and (N(plane["icp_status"]) == 0).all()
    x1, c1 = point["xyz1"], N(point["counts1"])
    for q in range(len(pairs)):
        v = int(c1[q])
        xq = x1[q:q + 1, :, :v].contiguous()
        a_point = float(reg.alignment_rmse(xq, gt[q:q + 1], point["icp_transform"][q:q + 1])[0])
        a_plane = float(reg.alignment_rmse(xq, gt[q:q + 1], plane["icp_transform"][q:q + 1])[0])
        print("scan pair %d: alignment rmse point %.4g (%d iterations), plane %.4g (%d)" % (
            q, a_point, int(point["icp_iterations"][q]), a_plane, int(plane["icp_iterations"][q])))
        assert a_plane <= a_point
    # the refinement is ops.icp from the solver's transform along normals2
    direct = ops.icp(plane["xyz1"], plane["xyz2"], plane["transform"], counts1=plane["counts1"],
                     counts2=plane["counts2"], normals2=plane["normals2"], **PLANE)
    for k, v in zip(ir.KEYS, direct):
        same(plane["icp_" + k], v, k)
    # fpfh_pairs on the same ragged clouds, and a normals2 of the caller's own is kept
    args = (plane["xyz1"], plane["normals1"], plane["xyz2"], plane["normals2"], 5 * cell, 100)
    kw = dict(search="grid", counts1=plane["counts1"], counts2=plane["counts2"])
    f_plane = reg.fpfh_pairs(*args, icp=PLANE, **kw)
    f_point = reg.fpfh_pairs(*args, icp={}, **kw)
    f_named = reg.fpfh_pairs(*args, icp=dict(estimation="point_to_point"), **kw)
    f_own = reg.fpfh_pairs(*args, icp=dict(PLANE, normals2=plane["normals2"].clone()), **kw)
    torch.cuda.synchronize()
    for k in f_plane:
        same(f_plane[k], plane[k], k)
        same(f_own[k], plane[k], k)
        same(f_named[k], f_point[k], k)
        same(f_point[k], point[k], k)
    assert (N(f_plane["icp_status"]) == 0).all()
    # icp_pairs and register_pairs pass the keywords through
    ip = reg.icp_pairs(plane["xyz1"], plane["xyz2"], plane["transform"], plane["counts1"],
                       plane["counts2"], normals2=plane["normals2"], **PLANE)
    for k in ir.KEYS:
        same(ip[k], plane["icp_" + k], k)
    rp = reg.register_pairs(plane["xyz1"], plane["xyz2"], plane["feat1"], plane["feat2"],
                            channel_major=True, counts1=plane["counts1"],
                            counts2=plane["counts2"],
                            icp=dict(PLANE, normals2=plane["normals2"]))
    for k in ir.KEYS:
        same(rp["icp_" + k], plane["icp_" + k], k)
    with pytest.raises(RuntimeError, match="needs normals2"):
        reg.register_pairs(plane["xyz1"], plane["xyz2"], plane["feat1"], plane["feat2"],
                           channel_major=True, counts1=plane["counts1"],
                           counts2=plane["counts2"], icp=PLANE)


def test_pair_extractor_register_fills_the_target_normals(dev):
    from clouds import gaussian_clouds
    from pcr_amd import ops
    from pcr_amd.registration import PairExtractor
    p, n, c, k, r = 2, 1024, 32, 16, 16
    xyz, nrm, feat = gaussian_clouds(2 * p, n, seed=47, c=c)
    rng = np.random.default_rng(p)
    rot = ir.rotation(rng, 25.0)
    for i in range(p):
        perm = rng.permutation(n)
        xyz[p + i] = (rot @ xyz[i])[:, perm]
        nrm[p + i] = (rot @ nrm[i])[:, perm]
        feat[p + i] = feat[i][:, perm]
    tx, tn, tf = (T(a.astype(np.float32), dev) for a in (xyz, nrm, feat))
    pe = PairExtractor(p, n, c, k, r, device=dev)
    kw = dict(hyps=128, inlier_dist=0.08, edge_ratio=0.9, refine_iters=2, seed=9)
    out = pe.register(tx, tn, tf, icp=dict(PLANE, max_dist=0.1, max_iters=30), **kw)
    torch.cuda.synchronize()
    direct = ops.icp(tx[:p], tx[p:], out["transform"], max_dist=0.1, max_iters=30,
                     normals2=tn[p:].contiguous(), **PLANE)
    for key, v in zip(ir.KEYS, direct):
        same(out["icp_" + key], v, key)
