"""GPU: pcr_icp_point_to_point (csrc/icp.hip) through ops.icp and
pcr_amd.registration against the numpy restatement of its contract
(tests/icp_restate.py).

Synthetic pairs (icp_restate.make_pair): source points uniform in the unit
ball, the target a permuted superset or subset moved by R a + t and rounded to
fp32; max_dist = 0.2 unless the case says otherwise.  Bounds:
  exact     corr, num_corr, iterations, status and fitness equal the
            restatement: the decisions are the same fp32 operations on both
            sides, under the asserted input condition that no convergence test
            lies within 1e-9 of its tolerance;
  rmse      1e-12 relative: fp64 sums of at most a few thousand non-negative
            terms in two orders;
  transform 1e-8 against the restatement: two fp64 solves (Horn / SVD) on
            O(1) data;
  recovery  1e-5 against the ground truth on the noise-free full-overlap
            cases: the fp32 rounding of the targets.
The workgroup's tile is 1024 source points (n1100 takes two) and the LDS chunk
8192 targets (n100_9000 takes two, n1030_8200 two of each)."""
import functools

import numpy as np
import pytest
import torch

import icp_restate as ir

pytestmark = pytest.mark.gpu

DEFAULTS = dict(max_dist=0.2, max_iters=200, rel_fitness=1e-6, rel_rmse=1e-6)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def perturbed(gt, degrees, seed):
    """gt with a further rotation of `degrees` about a random axis"""
    out = gt.copy()
    rng = np.random.default_rng(seed)
    for q in range(len(gt)):
        out[q, :3, :3] = ir.rotation(rng, degrees) @ gt[q, :3, :3]
    return out


# name -> (seed, p, n1, n2, make_pair keywords, icp keywords, recovers the ground truth)
CASES = {
    "tiny": (101, 1, 3, 5, {}, {}, True),
    "n64": (102, 2, 64, 64, {}, {}, True),
    "n256_300": (103, 3, 256, 300, dict(degrees=10.0, tnorm=0.05), {}, True),
    "n1100_1024": (104, 1, 1100, 1024, {}, {}, False),  # 76 sources have no counterpart
    "n300_5000": (105, 1, 300, 5000, {}, {}, True),
    "n100_9000": (106, 1, 100, 9000, {}, {}, True),
    "n1030_8200": (107, 1, 1030, 8200, {}, dict(max_iters=1), False),
    "dup": (108, 2, 128, 256, dict(dup=True), {}, True),
    "partial": (109, 2, 200, 140, dict(degrees=1.0, tnorm=0.01), dict(max_dist=0.05), False),
    "noise": (110, 2, 256, 256, dict(noise=0.004), {}, False),
    "init": (111, 2, 128, 128, dict(degrees=120.0, tnorm=0.3), {}, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    seed, p, n1, n2, mk, kw, _ = CASES[name]
    x1, x2, gt = ir.make_batch(seed, p, n1, n2, **mk)
    init = perturbed(gt, 3.0, seed) if name == "init" else None
    args = dict(DEFAULTS, **kw)
    exp = ir.icp(x1, x2, init, **args)
    return x1, x2, gt, init, args, exp


def run(dev, x1, x2, init=None, **kw):
    from pcr_amd import ops
    out = ops.icp(T(x1, dev), T(x2, dev), None if init is None else T(init, dev), **kw)
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
    assert got["transform"].dtype == np.float64 and dt <= 1e-8, name
    bottom = np.tile([0.0, 0.0, 0.0, 1.0], (len(exp["status"]), 1))
    assert np.array_equal(got["transform"][:, 3], bottom), name


def assert_self_consistent(x1, x2, got, max_dist):
    """Evaluate at the returned transform gives the returned corr / num_corr / rmse"""
    for q in range(len(x1)):
        ev = ir.evaluate(got["transform"][q, :3, :3], got["transform"][q, :3, 3],
                         np.ascontiguousarray(x1[q].T), np.ascontiguousarray(x2[q].T), max_dist)
        assert np.array_equal(ev["corr"], got["corr"][q]), q
        assert ev["num_corr"] == got["num_corr"][q] == (got["corr"][q] >= 0).sum(), q
        assert abs(ev["rmse"] - got["rmse"][q]) <= 1e-12 * max(ev["rmse"], 1e-300), q


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(dev, name):
    x1, x2, gt, init, args, exp = case(name)
    assert exp["conv_margin"] > 1e-9  # the input condition of the exact comparison
    got = run(dev, x1, x2, init, **args)
    assert_matches(got, exp, name)
    assert_self_consistent(x1, x2, got, args["max_dist"])
    n1, n2 = x1.shape[2], x2.shape[2]
    if name != "n1030_8200":
        assert (exp["status"] == 0).all() and (exp["iterations"] >= 1).all()
    if CASES[name][6]:
        err = np.abs(got["transform"] - gt).max()
        print("%s: recovery %.3g" % (name, err))
        assert err <= 1e-5
        assert (got["num_corr"] == n1).all()
    if name == "n1100_1024":
        assert (got["num_corr"] >= 1024).all()
    if name == "n1030_8200":
        assert exp["status"].tolist() == [2] and exp["iterations"].tolist() == [1]
    if name == "dup":
        assert (got["corr"] >= 0).all() and (got["corr"] < n2 // 2).all()
    if name == "partial":
        # a stray source may lie within 0.05 of some target
        assert (got["num_corr"] >= n2).all() and (got["num_corr"] <= n2 + 3).all()
        assert ((got["corr"] == -1).sum(axis=1) == n1 - got["num_corr"]).all()
    if name == "noise":
        # least squares over n points of noise sigma: about sigma * sqrt(3 / n) = 4e-4
        assert np.abs(got["transform"] - gt).max() <= 2e-3
        assert (got["rmse"] > 0.004).all() and (got["rmse"] < 0.012).all()
    if name == "init":
        # from the identity the 120 degree pair does not get there
        cold = run(dev, x1, x2, None, **args)
        assert np.abs(cold["transform"] - gt).max() > 0.1


def test_mixed_batch_statuses(dev):
    x1, x2, gt, _, args, exp = case("n64")
    far1, far2, _ = ir.make_batch(120, 1, 64, 64, tnorm=10.0)
    m1, m2 = np.concatenate((x1[:1], far1)), np.concatenate((x2[:1], far2))
    got = run(dev, m1, m2, **args)
    mexp = ir.icp(m1, m2, None, **args)
    assert mexp["conv_margin"] > 1e-9
    assert_matches(got, mexp, "mixed")
    assert got["status"].tolist() == [0, 1] and got["iterations"][1] == 0
    assert np.array_equal(got["transform"][1], np.eye(4))
    assert (got["corr"][1] == -1).all() and got["num_corr"][1] == 0
    assert got["fitness"][1] == 0.0 and got["rmse"][1] == 0.0
    # the far pair keeps a given init as it is
    init = np.stack((np.eye(4), ir.motion(np.random.default_rng(1), 30.0, 0.5)))
    kept = run(dev, m1, m2, init, **args)
    assert kept["status"][1] == 1 and np.array_equal(kept["transform"][1], init[1])
    # one iteration: the limit
    one = run(dev, m1, m2, **dict(args, max_iters=1))
    oexp = ir.icp(m1, m2, None, **dict(args, max_iters=1))
    assert oexp["conv_margin"] > 1e-9
    assert_matches(one, oexp, "max_iters=1")
    assert one["status"].tolist() == [2, 1] and one["iterations"].tolist() == [1, 0]
    # no iteration: the evaluation of the init
    zero = run(dev, m1, m2, **dict(args, max_iters=0))
    assert_matches(zero, ir.icp(m1, m2, None, **dict(args, max_iters=0)), "max_iters=0")
    assert zero["status"].tolist() == [2, 2] and zero["iterations"].tolist() == [0, 0]
    assert np.array_equal(zero["transform"], np.tile(np.eye(4), (2, 1, 1)))
    assert_self_consistent(m1, m2, zero, args["max_dist"])


def test_argument_checks(dev):
    from pcr_amd import ops
    x1, x2, gt, _, args, exp = case("n64")
    t1, t2 = T(x1, dev), T(x2, dev)
    good = T(np.tile(np.eye(4), (2, 1, 1)), dev)
    bad = {"float32 init": good.float(), "init of another batch": good[:1],
           "3 x 4 init": good[:, :3].contiguous(), "strided init": good.transpose(1, 2),
           "host init": good.cpu()}
    for what, init in bad.items():
        with pytest.raises(RuntimeError):
            ops.icp(t1, t2, init)
    for a, b in ((t1[:1], t2), (t1.double(), t2), (t1.transpose(1, 2), t2), (t1[:, :2], t2)):
        with pytest.raises(RuntimeError):
            ops.icp(a, b)
    for kw in (dict(max_dist=0.0), dict(max_iters=-1), dict(rel_rmse=-1.0)):
        with pytest.raises(RuntimeError, match="icp"):
            ops.icp(t1, t2, **kw)
    ops.icp(t1, t2, good)  # and the good one is taken
    torch.cuda.synchronize()


def test_deterministic_and_batch_independent(dev):
    x1, x2, gt, _, args, exp = case("n256_300")
    one, two = run(dev, x1, x2, **args), run(dev, x1, x2, **args)
    for k in ir.KEYS:
        assert one[k].tobytes() == two[k].tobytes(), k
    for q in range(len(x1)):
        alone = run(dev, x1[q:q + 1], x2[q:q + 1], **args)
        for k in ir.KEYS:
            assert alone[k][0].tobytes() == one[k][q].tobytes(), (q, k)
    x1, x2, gt, _, args, exp = case("n1100_1024")  # the tiled path
    one, two = run(dev, x1, x2, **args), run(dev, x1, x2, **args)
    for k in ir.KEYS:
        assert one[k].tobytes() == two[k].tobytes(), k


def test_side_stream_overwrites_poisoned_outputs(dev):
    """the C ABI on a stream of its own, into buffers pre-filled with garbage"""
    from pcr_amd import _lib
    x1, x2, gt, _, args, exp = case("n64")
    far1, far2, _ = ir.make_batch(120, 1, 64, 64, tnorm=10.0)
    m1, m2 = np.concatenate((x1, far1)), np.concatenate((x2, far2))
    ref = run(dev, m1, m2, **args)
    p, n1, n2 = 3, 64, 64
    t1, t2 = T(m1, dev), T(m2, dev)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    bufs = dict(transform=torch.full((p, 4, 4), float("nan"), **f64),
                corr=torch.full((p, n1), -77, **i32), num_corr=torch.full((p,), -77, **i32),
                fitness=torch.full((p,), float("nan"), **f64),
                rmse=torch.full((p,), float("nan"), **f64),
                iterations=torch.full((p,), -77, **i32), status=torch.full((p,), -77, **i32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    _lib.check(_lib.load().pcr_icp_point_to_point(
        t1.data_ptr(), t2.data_ptr(), p, n1, n2, None, args["max_dist"], args["max_iters"],
        args["rel_fitness"], args["rel_rmse"], *[bufs[k].data_ptr() for k in ir.KEYS],
        side.cuda_stream), "icp")
    side.synchronize()
    for k in ir.KEYS:
        assert N(bufs[k]).tobytes() == ref[k].tobytes(), k


def wrong_match_pairs(seed, p, n, c, wrong, noise):
    """pairs whose features match every point, a fraction `wrong` of them to
    the wrong point: feat2 rows are feat1 rows, deranged within the wrong set"""
    rng = np.random.default_rng(seed)
    x1, x2 = np.empty((p, 3, n), np.float32), np.empty((p, 3, n), np.float32)
    gt = np.stack([ir.motion(rng, 40.0, 0.3) for _ in range(p)])
    feat1 = rng.standard_normal((p, n, c)).astype(np.float32)
    feat2 = np.empty_like(feat1)
    for q in range(p):
        a = ir.ball(rng, n).astype(np.float32)
        src = rng.permutation(n)  # the source of target j
        moved = a[src].astype(np.float64) @ gt[q, :3, :3].T + gt[q, :3, 3]
        x1[q], x2[q] = a.T, (moved + rng.normal(0, 1, (n, 3)) * noise).T
        bad = rng.permutation(n)[:int(wrong * n)]
        src[bad] = src[np.roll(bad, 1)]
        feat2[q] = feat1[q][src]
    return x1, x2, gt, feat1, feat2


def test_register_pairs_refines_ransac(dev):
    from pcr_amd.registration import alignment_rmse, icp_pairs, register_pairs, rre_rte
    p, n = 4, 512
    x1, x2, gt, f1, f2 = wrong_match_pairs(130, p, n, 32, 0.55, 0.004)
    tx1, tx2, tf1, tf2, tgt = (T(a, dev) for a in (x1, x2, f1, f2, gt))
    kw = dict(hyps=512, inlier_dist=0.02, edge_ratio=0.9, refine_iters=2, seed=5)
    plain = register_pairs(tx1, tx2, tf1, tf2, **kw)
    both = register_pairs(tx1, tx2, tf1, tf2, icp={}, **kw)
    torch.cuda.synchronize()
    icp_keys = {"icp_" + k for k in ir.KEYS}
    assert set(both) == set(plain) | icp_keys
    for k, v in plain.items():
        if v is not None:
            assert N(both[k]).tobytes() == N(v).tobytes(), k
    assert (N(plain["reg_status"]) == 0).all() and (N(both["icp_status"]) == 0).all()
    rre0, rte0 = rre_rte(tgt, plain["transform"])
    rre1, rte1 = rre_rte(tgt, both["icp_transform"])
    print("RRE %.4g -> %.4g degrees, RTE %.4g -> %.4g" % (
        rre0.mean().item(), rre1.mean().item(), rte0.mean().item(), rte1.mean().item()))
    assert rre1.mean().item() <= rre0.mean().item()
    assert rte1.mean().item() <= rte0.mean().item()
    a0 = alignment_rmse(tx1, tgt, plain["transform"])
    a1 = alignment_rmse(tx1, tgt, both["icp_transform"])
    assert a1.mean().item() <= a0.mean().item()
    # the refinement is ops.icp from the RANSAC transform; icp_pairs is the same call
    direct = icp_pairs(tx1, tx2, plain["transform"])
    for k in ir.KEYS:
        assert N(direct[k]).tobytes() == N(both["icp_" + k]).tobytes(), k
    exp = ir.icp(x1, x2, N(plain["transform"]), **DEFAULTS)
    assert exp["conv_margin"] > 1e-9
    assert_matches({k: N(direct[k]) for k in ir.KEYS}, exp, "refine")


def test_pair_extractor_register_with_icp(dev):
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
    plain = {key: v.clone() for key, v in pe.register(tx, tn, tf, **kw).items()}
    out = pe.register(tx, tn, tf, icp=dict(max_dist=0.1, max_iters=30), **kw)
    torch.cuda.synchronize()
    assert set(out) == set(plain) | {"icp_" + key for key in ir.KEYS}
    for key, v in plain.items():
        assert N(out[key]).tobytes() == N(v).tobytes(), key
    direct = ops.icp(tx[:p], tx[p:], out["transform"], max_dist=0.1, max_iters=30)
    for key, v in zip(ir.KEYS, direct):
        assert N(out["icp_" + key]).tobytes() == N(v).tobytes(), key
    assert tuple(out["icp_transform"].shape) == (p, 4, 4)
    assert tuple(out["icp_corr"].shape) == (p, n)
