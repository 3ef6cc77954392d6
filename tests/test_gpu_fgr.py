"""GPU: pcr_fgr (csrc/fgr.hip) through ops.fgr and pcr_amd.registration against
the numpy restatement of its contract (tests/fgr_restate.py).

Synthetic pairs (fgr_restate.make_pair): source points uniform in the unit
ball, the target a permuted superset moved by 40 degrees and |t| = 0.5 and
rounded to fp32; slot s pairs source s with its counterpart, a stated fraction
of the slots with a random target instead.  Bounds:
  exact     slots, num_corr, num_trials, status and mu equal the restatement:
            the tuple test and the centroids' sums are the same fp64
            operations in the same order on both sides;
  transform 1e-8 against the restatement (two fp64 solves on O(1) data, as in
            4.8a / 4.8b), under the asserted input condition that the
            restatement with its sums ascending and descending agrees to 1e-11;
  recovery  1e-5 against the ground truth where every match is correct: the
            fp32 rounding of the targets.
With wrong matches the distance to the ground truth is printed, not bounded.
The tuple kernel walks rounds of 1024 trials; the loop kernel keeps up to 3072
correspondences in LDS (the capacity `past_lds` exceeds by 28) and re-reads a
longer list from the workspace every iteration."""
import functools

import numpy as np
import pytest
import torch

import fgr_restate as fr
import icp_restate as ir

pytestmark = pytest.mark.gpu

LDS_CAPACITY = 3072

# name -> (seed, p, n1, n2, make_pair keywords, fgr keywords, every match correct)
CASES = {
    "tiny": (201, 1, 16, 16, {}, dict(max_tuples=0), True),
    "nine": (202, 1, 32, 32, dict(m=9), dict(max_tuples=0), False),
    "cap_in_round": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100), False),
    "exhausted": (204, 1, 64, 64, dict(wrong=0.7), {}, False),
    "full_list": (205, 2, 1024, 1100, dict(wrong=0.55), {}, False),
    "past_lds": (206, 1, LDS_CAPACITY + 28, LDS_CAPACITY + 28, {}, dict(max_tuples=0), True),
    "clean_tuples": (207, 2, 200, 230, dict(degrees=150.0), dict(max_tuples=60), True),
    "absolute": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100, absolute_scale=True),
                 False),
    "fixed_mu": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100, decrease_mu=False),
                 False),
    "no_step": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100, iterations=0), False),
    "one_step": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100, iterations=1), False),
    "seed": (203, 2, 256, 256, dict(wrong=0.3), dict(max_tuples=100, seed=12345), False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    seed, p, n1, n2, mk, kw, _ = CASES[name]
    batch = fr.make_batch(seed, p, n1, n2, **mk)
    exp, gap = fr.order_gap(*batch[:5], **kw)
    return batch, kw, exp, gap


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def run(dev, x1, x2, i1, i2, count, **kw):
    from pcr_amd import ops
    out = ops.fgr(*(T(a, dev) for a in (x1, x2, i1, i2, count)), **kw)
    torch.cuda.synchronize()
    return dict(zip(fr.KEYS, (N(o) for o in out)))


def assert_matches(got, exp, name=""):
    for k in ("status", "num_corr", "num_trials", "slots"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (name, k)
    assert got["mu"].dtype == np.float64 and np.array_equal(got["mu"], exp["mu"]), name
    dt = np.abs(got["transform"] - exp["transform"]).max()
    print("%s: K %s, trials %s, mu %s, transform %.3g" % (
        name, got["num_corr"].tolist(), got["num_trials"].tolist(), got["mu"].tolist(), dt))
    assert got["transform"].dtype == np.float64 and dt <= 1e-8, name
    bottom = np.tile([0.0, 0.0, 0.0, 1.0], (len(exp["status"]), 1))
    assert np.array_equal(got["transform"][:, 3], bottom), name


def report_errors(name, gt, got, exp):
    for who, tr in (("kernel", got["transform"]), ("restatement", exp["transform"])):
        rre, rte = fr.rre_rte(gt, tr)
        print("%s %s: RRE %s degrees, RTE %s" % (name, who, rre.tolist(), rte.tolist()))


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(dev, name):
    batch, kw, exp, gap = case(name)
    x1, x2, i1, i2, count, gt = batch
    assert gap <= 1e-11  # the input condition of the transform's bound
    got = run(dev, *batch[:5], **kw)
    assert_matches(got, exp, name)
    report_errors(name, gt, got, exp)
    p, n1 = x1.shape[0], x1.shape[2]
    if CASES[name][6]:
        err = np.abs(got["transform"] - gt).max()
        print("%s: recovery %.3g" % (name, err))
        assert (got["status"] == 0).all() and err <= 1e-5
    if name in ("tiny", "past_lds"):
        assert (got["num_corr"] == n1).all() and (got["num_trials"] == 0).all()
        assert np.array_equal(got["slots"], np.tile(np.arange(n1, dtype=np.int32), (p, 1)))
    if name == "nine":
        assert got["status"].tolist() == [1] and got["num_corr"].tolist() == [9]
        assert got["num_trials"].tolist() == [0] and got["mu"].tolist() == [0.0]
        assert np.array_equal(got["transform"][0], np.eye(4))
        assert np.array_equal(got["slots"][0], np.r_[np.arange(9), np.full(n1 - 9, -1)])
    if name == "cap_in_round":
        # the cap falls inside the first round of 1024 trials
        assert (got["num_corr"] == 300).all() and (got["num_trials"] < 1024).all()
        assert (got["slots"] >= 0).all() and (got["status"] == 0).all()
    if name == "exhausted":
        k = int(got["num_corr"][0])
        assert got["num_trials"].tolist() == [6400] and 10 <= k < 3000 and k % 3 == 0
        assert (got["slots"][0, :k] >= 0).all() and (got["slots"][0, k:] == -1).all()
    if name == "full_list":
        # several rounds per pair, the list and the LDS at their fullest
        assert (got["num_corr"] == 3000).all() and (got["num_trials"] > 2048).all()
        assert (got["num_trials"] < 102400).all() and (got["status"] == 0).all()
    if name == "absolute":
        assert ((got["mu"] > 0.08 / 1.4) & (got["mu"] <= 0.08)).all()
    if name == "fixed_mu":
        assert (got["mu"] == 1.0).all()
    if name == "no_step":
        assert (got["mu"] == 1.0).all()
        assert np.array_equal(got["transform"][:, :3, :3], np.tile(np.eye(3), (p, 1, 1)))
    if name == "one_step":
        assert (got["mu"] == 1.0 / 1.4).all()
    if name == "seed":
        other = case("cap_in_round")[2]
        assert not np.array_equal(got["slots"], other["slots"])


def test_too_few_with_the_tuple_test(dev):
    """M = 2 and count = 0: no trials are made, num_trials is H = 100 M"""
    x1, x2, i1, i2, count, gt = fr.make_batch(210, 2, 32, 32)
    count = np.array([2, 0], np.int32)
    got = run(dev, x1, x2, i1, i2, count)
    assert_matches(got, fr.fgr(x1, x2, i1, i2, count), "too few")
    assert got["status"].tolist() == [1, 1] and got["num_corr"].tolist() == [0, 0]
    assert got["num_trials"].tolist() == [200, 0] and got["mu"].tolist() == [0.0, 0.0]
    assert np.array_equal(got["transform"], np.tile(np.eye(4), (2, 1, 1)))
    assert (got["slots"] == -1).all() and got["slots"].shape == (2, 3000)


def test_bad_pairs_do_not_touch_the_others(dev):
    """a NaN point, coincident clouds (status 2) and a one-point target
    (status 3) behind two good pairs, which keep their bits"""
    x1, x2, i1, i2, count, gt = fr.make_batch(211, 5, 64, 64, wrong=0.2)
    x1[2, 1, 7] = np.nan
    x1[3], x2[3] = 0.25, -0.5
    x2[4] = -0.5
    kw = dict(max_tuples=0)
    exp, gap = fr.order_gap(x1, x2, i1, i2, count, **kw)
    assert gap <= 1e-11 and exp["status"].tolist() == [0, 0, 2, 2, 3]
    got = run(dev, x1, x2, i1, i2, count, **kw)
    assert_matches(got, exp, "bad pairs")
    assert got["mu"][2:].tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(got["transform"][2:4], np.tile(np.eye(4), (2, 1, 1)))
    good = run(dev, x1[:2], x2[:2], i1[:2], i2[:2], count[:2], **kw)
    for k in fr.KEYS:
        assert good[k].tobytes() == got[k][:2].tobytes(), k
    # under the tuple test the triples away from the NaN point still pass
    # (status 2 again); no triple of the other two does: status 1
    tup = run(dev, x1, x2, i1, i2, count, max_tuples=50)
    texp = fr.fgr(x1, x2, i1, i2, count, max_tuples=50)
    assert_matches(tup, texp, "bad pairs, tuple test")
    assert tup["status"][2:].tolist() == [2, 1, 1] and tup["num_corr"][2:].tolist() == [150, 0, 0]
    good = run(dev, x1[:2], x2[:2], i1[:2], i2[:2], count[:2], max_tuples=50)
    for k in fr.KEYS:
        assert good[k].tobytes() == tup[k][:2].tobytes(), k


def test_deterministic_and_batch_independent(dev):
    for name in ("full_list", "cap_in_round"):
        batch, kw, exp, gap = case(name)
        one, two = run(dev, *batch[:5], **kw), run(dev, *batch[:5], **kw)
        for k in fr.KEYS:
            assert one[k].tobytes() == two[k].tobytes(), (name, k)
        # the sampler takes the pair's index: pair 0 alone is pair 0 of the batch
        alone = run(dev, *(a[:1] for a in batch[:5]), **kw)
        for k in fr.KEYS:
            assert alone[k][0].tobytes() == one[k][0].tobytes(), (name, k)
    # without the tuple test every pair is the same alone
    batch = fr.make_batch(212, 3, 300, 300, wrong=0.3)
    one = run(dev, *batch[:5], max_tuples=0)
    for q in range(3):
        alone = run(dev, *(a[q:q + 1] for a in batch[:5]), max_tuples=0)
        for k in fr.KEYS:
            assert alone[k][0].tobytes() == one[k][q].tobytes(), (q, k)


def test_argument_checks(dev):
    from pcr_amd import ops
    batch, kw, exp, gap = case("cap_in_round")
    t = [T(a, dev) for a in batch[:5]]
    for i, bad in ((0, t[0].double()), (0, t[0][:1]), (1, t[1][:, :2]), (2, t[2].long()),
                   (3, t[3][:, :100]), (4, t[4][:1]), (2, t[2].cpu())):
        args = list(t)
        args[i] = bad
        with pytest.raises(RuntimeError):
            ops.fgr(*args)
    for bad in (dict(iterations=-1), dict(iterations=100001), dict(division_factor=1.0),
                dict(tuple_scale=1.0), dict(tuple_scale=-0.5), dict(max_tuples=-1),
                dict(trials_per_corr=1 << 24)):
        with pytest.raises(RuntimeError, match="fgr"):
            ops.fgr(*t, **bad)
    small = torch.empty(256, dtype=torch.uint8, device=dev)
    out = ops.fgr(*t, workspace=small, **kw)  # too small a workspace is replaced
    torch.cuda.synchronize()
    assert np.array_equal(N(out[1]), exp["slots"])


def test_side_stream_overwrites_poisoned_outputs(dev):
    """the C ABI on a stream of its own, into buffers pre-filled with garbage"""
    from pcr_amd import _lib
    batch, kw, exp, gap = case("cap_in_round")
    ref = run(dev, *batch[:5], **kw)
    t = [T(a, dev) for a in batch[:5]]
    p, n1, n2, kcap = 2, 256, 256, 300
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    bufs = dict(transform=torch.full((p, 4, 4), float("nan"), **f64),
                slots=torch.full((p, kcap), -77, **i32), num_corr=torch.full((p,), -77, **i32),
                num_trials=torch.full((p,), -77, **i32), mu=torch.full((p,), float("nan"), **f64),
                status=torch.full((p,), -77, **i32))
    lib = _lib.load()
    ws = torch.full((lib.pcr_fgr_workspace_size(p, n1, 100),), 0xFF, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    a = dict(fr.DEFAULTS, **kw)
    _lib.check(lib.pcr_fgr(
        *[x.data_ptr() for x in t[:2]], p, n1, n2, *[x.data_ptr() for x in t[2:]],
        a["max_corr_dist"], a["iterations"], a["division_factor"], int(a["decrease_mu"]),
        a["tuple_scale"], a["max_tuples"], a["trials_per_corr"], int(a["absolute_scale"]),
        a["seed"], *[bufs[k].data_ptr() for k in fr.KEYS], ws.data_ptr(), ws.numel(),
        side.cuda_stream), "fgr")
    side.synchronize()
    for k in fr.KEYS:
        assert N(bufs[k]).tobytes() == ref[k].tobytes(), k


# ------------------------------------------------------------ end to end
def feature_pairs(seed, p, n, c, wrong):
    """noise-free full-overlap pairs whose features match every point, a
    fraction `wrong` of them to the wrong point (feat2 rows are feat1 rows,
    deranged within the wrong set) -> clouds, gt, features and the matching
    they determine: idx1 = 0 .. n-1, idx2"""
    rng = np.random.default_rng(seed)
    x1, x2 = np.empty((p, 3, n), np.float32), np.empty((p, 3, n), np.float32)
    gt = np.stack([ir.motion(rng, 40.0, 0.3) for _ in range(p)])
    feat1 = rng.standard_normal((p, n, c)).astype(np.float32)
    feat2 = np.empty_like(feat1)
    idx2 = np.empty((p, n), np.int32)
    for q in range(p):
        a = ir.ball(rng, n).astype(np.float32)
        src = rng.permutation(n)  # the source of target j
        x1[q], x2[q] = a.T, (a[src].astype(np.float64) @ gt[q, :3, :3].T + gt[q, :3, 3]).T
        bad = rng.permutation(n)[:int(wrong * n)]
        src[bad] = src[np.roll(bad, 1)]
        feat2[q] = feat1[q][src]
        idx2[q, src] = np.arange(n)
    idx1 = np.tile(np.arange(n, dtype=np.int32), (p, 1))
    return x1, x2, gt, feat1, feat2, idx1, idx2


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    p, n = 2, 256
    x1, x2, gt, f1, f2, idx1, idx2 = feature_pairs(220, p, n, 32, 0.55)
    count = np.full(p, n, np.int32)
    exp, gap = fr.order_gap(x1, x2, idx1, idx2, count)
    iexp = ir.icp(x1, x2, exp["transform"], max_dist=0.2, max_iters=200, rel_fitness=1e-6,
                  rel_rmse=1e-6)
    return (x1, x2, gt, f1, f2, idx1, idx2, count), exp, gap, iexp


def test_register_pairs_with_the_fgr_solver(dev):
    from pcr_amd import ops
    from pcr_amd.registration import fgr_pairs, register_pairs
    (x1, x2, gt, f1, f2, idx1, idx2, count), exp, gap, iexp = end_to_end_case()
    # the input conditions: a well conditioned loop, and a restatement chain
    # fgr -> icp that itself reaches the ground truth
    assert gap <= 1e-11 and (exp["status"] == 0).all()
    assert iexp["conv_margin"] > 1e-9 and (iexp["status"] == 0).all()
    assert np.abs(iexp["transform"] - gt).max() <= 1e-5
    tx1, tx2, tf1, tf2 = (T(a, dev) for a in (x1, x2, f1, f2))
    plain = fgr_pairs(tx1, tx2, tf1, tf2)
    both = register_pairs(tx1, tx2, tf1, tf2, solver="fgr", icp={})
    torch.cuda.synchronize()
    fgr_keys = {"idx1", "idx2", "count", "transform", "slots", "num_corr", "num_trials", "mu",
                "reg_status"}
    assert set(plain) == fgr_keys
    assert set(both) == fgr_keys | {"icp_" + k for k in ir.KEYS}
    for k, v in plain.items():
        assert N(both[k]).tobytes() == N(v).tobytes(), k
    assert np.array_equal(N(plain["idx1"]), idx1) and np.array_equal(N(plain["idx2"]), idx2)
    assert np.array_equal(N(plain["count"]), count)
    # the solver is ops.fgr on the matching's output
    direct = ops.fgr(tx1, tx2, plain["idx1"], plain["idx2"], plain["count"])
    for k, v in zip(("transform", "slots", "num_corr", "num_trials", "mu", "reg_status"), direct):
        assert N(plain[k]).tobytes() == N(v).tobytes(), k
    got = {k: N(plain["reg_status" if k == "status" else k]) for k in fr.KEYS}
    assert_matches(got, exp, "end to end")
    report_errors("end to end", gt, got, exp)
    # the refinement is ops.icp from the FGR transform, and reaches the ground truth
    refined = ops.icp(tx1, tx2, plain["transform"])
    for k, v in zip(ir.KEYS, refined):
        assert N(both["icp_" + k]).tobytes() == N(v).tobytes(), k
    err = np.abs(N(both["icp_transform"]) - gt).max()
    print("end to end: after ICP %.3g" % err)
    assert (N(both["icp_status"]) == 0).all() and err <= 1e-5
    # the default solver is what it was: ops.rigid_ransac on the matching, the same keys
    kw = dict(hyps=256, inlier_dist=0.02, seed=3)
    default = register_pairs(tx1, tx2, tf1, tf2, **kw)
    named = register_pairs(tx1, tx2, tf1, tf2, solver="ransac", **kw)
    ransac = ops.rigid_ransac(tx1, tx2, default["idx1"], default["idx2"], default["count"], **kw)
    assert list(default) == ["idx1", "idx2", "count", "transform", "inliers", "num_inliers",
                             "best_hyp", "reg_status"]
    for k, v in zip(("transform", "inliers", "num_inliers", "best_hyp", "reg_status"), ransac):
        assert N(default[k]).tobytes() == N(v).tobytes() == N(named[k]).tobytes(), k


def test_pair_extractor_register_with_the_fgr_solver(dev):
    from clouds import gaussian_clouds
    from pcr_amd import ops
    from pcr_amd.registration import PairExtractor
    p, n, c, k, r = 2, 1024, 32, 16, 16
    xyz, nrm, feat = gaussian_clouds(2 * p, n, seed=48, c=c)
    rng = np.random.default_rng(p)
    rot = ir.rotation(rng, 25.0)
    for i in range(p):
        perm = rng.permutation(n)
        xyz[p + i] = (rot @ xyz[i])[:, perm]
        nrm[p + i] = (rot @ nrm[i])[:, perm]
        feat[p + i] = feat[i][:, perm]
    tx, tn, tf = (T(a.astype(np.float32), dev) for a in (xyz, nrm, feat))
    pe = PairExtractor(p, n, c, k, r, device=dev)
    out = pe.register(tx, tn, tf, solver="fgr", icp=dict(max_dist=0.1, max_iters=30),
                      max_tuples=200)
    torch.cuda.synchronize()
    assert {"transform", "slots", "num_corr", "num_trials", "mu", "reg_status", "icp_transform",
            "devox", "idx1"} <= set(out)
    direct = ops.fgr(tx[:p], tx[p:], out["idx1"], out["idx2"], out["count"], max_tuples=200)
    for key, v in zip(("transform", "slots", "num_corr", "num_trials", "mu", "reg_status"),
                      direct):
        assert N(out[key]).tobytes() == N(v).tobytes(), key
    assert tuple(out["slots"].shape) == (p, 600)
