"""GPU: pcr_teaser (csrc/teaser.hip) through ops.teaser and pcr_amd.registration
against the numpy restatement of its contract (tests/teaser_restate.py,
DESIGN.md 4.8d).

Synthetic pairs (teaser_restate.make_pair): source points uniform in the unit
ball, the target a permuted superset moved by 40 degrees and |t| = 0.5 and
rounded to fp32; slot s pairs source s with its counterpart, a stated fraction
of the slots with another target instead.  Bounds, those of the C run in
tests/test_teaser_cpu.py:
  exact     clique, clique_size, inliers, num_inliers, iterations and status
            equal the restatement: the edge test, the weights and the
            endpoints are the same fp64 operations on both sides;
  transform 1e-8 against the restatement (fp64 solves on O(1) data, as in
            4.8a-c), under the asserted input condition that the restatement
            with its sums ascending and descending agrees to 1e-11 and in
            every exact output, so no near-tie decides one;
  recovery  1e-5 against the ground truth on planted pairs (noise-free
            inliers): the fp32 rounding of the targets.
The clique kernel stages the bit rows in LDS up to n1 = 1024 (`past_lds` is
above it) and holds a row as one 64-bit word per lane (63 / 64 / 65 / 130
slots: one, one, two and three words); the solve kernel's 512 threads walk the
K (K - 1) / 2 TIMs in rounds."""
import functools

import numpy as np
import pytest
import torch

import icp_restate as ir
import teaser_restate as tr

pytestmark = pytest.mark.gpu

LDS_ROWS = 1024
SOLVE_THREADS = 512

# name -> (seed, p, n1, n2, make_pair keywords, teaser keywords, planted)
CASES = {
    "m63": (301, 1, 63, 80, dict(wrong=0.5), {}, True),
    "m64": (302, 2, 64, 64, dict(wrong=0.5), {}, True),
    "m65": (303, 1, 65, 70, dict(wrong=0.55), {}, True),
    "m130": (304, 2, 130, 150, dict(wrong=0.3), {}, True),
    "wrong90": (305, 1, 400, 400, dict(wrong=0.9), {}, True),
    "past_lds": (306, 1, LDS_ROWS + 76, LDS_ROWS + 76, dict(wrong=0.9), {}, True),
    "tims": (307, 1, 66, 66, dict(wrong=0.5), {}, True),
    "noisy": (308, 2, 150, 150, dict(wrong=0.4, noise=0.02), {}, False),
    "capped": (309, 2, 160, 160, dict(wrong=0.5), dict(seeds=5), False),
    "all_slots": (310, 2, 100, 100, dict(wrong=0.3), dict(inlier_selection=False), False),
    "limit": (310, 2, 100, 100, dict(wrong=0.3), dict(inlier_selection=False, max_iters=3),
              False),
    "loose": (311, 1, 90, 90, dict(wrong=0.5, noise=0.06),
              dict(noise_bound=0.05, cbar2=1.5, gnc_factor=1.2, cost_threshold=1e-9), False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    seed, p, n1, n2, mk, kw, _ = CASES[name]
    batch = tr.make_batch(seed, p, n1, n2, **mk)
    exp, gap = tr.order_gap(*batch[:5], **kw)
    return batch, kw, exp, gap


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def run(dev, x1, x2, i1, i2, count, **kw):
    from pcr_amd import ops
    out = ops.teaser(*(T(a, dev) for a in (x1, x2, i1, i2, count)), **kw)
    torch.cuda.synchronize()
    return dict(zip(tr.KEYS, (N(o) for o in out)))


def assert_matches(got, exp, name=""):
    for k in tr.KEYS[1:]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (name, k)
    dt = np.abs(got["transform"] - exp["transform"]).max()
    print("%s: K %s, inliers %s, iterations %s, status %s, transform %.3g" % (
        name, got["clique_size"].tolist(), got["num_inliers"].tolist(),
        got["iterations"].tolist(), got["status"].tolist(), dt))
    assert got["transform"].dtype == np.float64 and dt <= 1e-8, name
    bottom = np.tile([0.0, 0.0, 0.0, 1.0], (len(exp["status"]), 1))
    assert np.array_equal(got["transform"][:, 3], bottom), name


def report_errors(name, gt, got, exp):
    for who, t in (("kernel", got["transform"]), ("restatement", exp["transform"])):
        rre, rte = tr.rre_rte(gt, t)
        print("%s %s: RRE %s degrees, RTE %s" % (name, who, rre.tolist(), rte.tolist()))


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(dev, name):
    batch, kw, exp, gap = case(name)
    x1, x2, i1, i2, count, gt, planted = batch
    assert gap <= 1e-11  # the input condition of the transform's bound
    got = run(dev, *batch[:5], **kw)
    assert_matches(got, exp, name)
    report_errors(name, gt, got, exp)
    p, n1 = x1.shape[0], x1.shape[2]
    ks = got["clique_size"]
    for q in range(p):
        cl = got["clique"][q]
        assert (np.diff(cl[:ks[q]]) > 0).all() and (cl[ks[q]:] == -1).all()
        assert got["inliers"][q].sum() == got["num_inliers"][q]
        assert got["inliers"][q][cl[:ks[q]]].sum() == got["num_inliers"][q]
    if CASES[name][6]:
        # the conditions on planted pairs, met by the restatement itself
        for q in range(p):
            assert np.array_equal(exp["clique"][q, :exp["clique_size"][q]], planted[q])
        assert np.abs(exp["transform"] - gt).max() <= 1e-5
        err = np.abs(got["transform"] - gt).max()
        print("%s: recovery %.3g" % (name, err))
        assert (got["status"] == 0).all() and err <= 1e-5
        assert (got["iterations"] == 1).all() and np.array_equal(got["num_inliers"], ks)
    if name == "tims":
        tims = int(ks[0]) * (int(ks[0]) - 1) // 2
        assert tims > SOLVE_THREADS and tims % SOLVE_THREADS != 0
    if name in ("noisy", "all_slots", "loose"):
        assert (got["status"] == 0).all() and (got["iterations"] > 3).all()  # the GNC loop ran
    if name in ("all_slots", "limit"):
        assert np.array_equal(got["clique"], np.tile(np.arange(n1, dtype=np.int32), (p, 1)))
    if name == "all_slots":
        for q in range(p):
            assert np.array_equal(np.nonzero(got["inliers"][q])[0], planted[q])
    if name == "limit":
        assert (got["status"] == 3).all() and (got["iterations"] == 3).all()
    if name == "capped":
        full = tr.teaser(*batch[:5])
        assert ((3 <= ks) & (ks <= full["clique_size"])).all()


def test_small_graphs_reach_the_exact_maximum(dev):
    """graphs of at most 40 vertices: the kernel's clique is as large as the
    exact maximum clique (brute force on the restatement's graph)"""
    for seed, n, wrong in ((320, 12, 0.5), (321, 24, 0.7), (322, 40, 0.55), (323, 40, 0.9)):
        x1, x2, i1, i2, count, gt, planted = tr.make_batch(seed, 2, n, 3 * n, wrong=wrong)
        exp, gap = tr.order_gap(x1, x2, i1, i2, count)
        assert gap <= 1e-11
        got = run(dev, x1, x2, i1, i2, count)
        assert_matches(got, exp, "small %d" % n)
        for q in range(2):
            a32 = np.ascontiguousarray(x1[q][:, i1[q]].T)
            b32 = np.ascontiguousarray(x2[q][:, i2[q]].T)
            adj = tr.graph(a32, b32, tr.bounds(0.02, 1.0)[0])
            cl = got["clique"][q, :got["clique_size"][q]]
            assert adj[np.ix_(cl, cl)].sum() == len(cl) * (len(cl) - 1)  # a clique
            assert len(cl) == tr.max_clique_size(adj)


def mixed_batch(all_wrong=True):
    """good pairs 0, 3, 8 among bad ones: count 0 / 1 / 2, every match wrong (a
    target three times the size, deranged: no three slots agree; it is a case
    of the clique search, and without the search a loop over nothing but
    wrong TIMs whose end hangs on the last bit of its sums, so that run leaves
    pair 5 a good one), a NaN point, a cloud of coincident points"""
    x1, x2, i1, i2, count, gt, planted = tr.make_batch(330, 9, 96, 96, wrong=0.5)
    count[1], count[2], count[4] = 0, 1, 2
    count[3] = 70
    if all_wrong:
        i2[5] = (i2[5] + 1 + np.arange(96) % 7) % 96
        x2[5] *= 3.0
    x1[6, 1, 7] = np.nan
    x2[7] = -0.5
    return x1, x2, i1, i2, count


def test_bad_pairs_do_not_touch_the_others(dev):
    for kw in ({}, dict(inlier_selection=False)):
        x1, x2, i1, i2, count = mixed_batch(all_wrong=not kw)
        exp, gap = tr.order_gap(x1, x2, i1, i2, count, **kw)
        assert gap <= 1e-11
        got = run(dev, x1, x2, i1, i2, count, **kw)
        assert_matches(got, exp, "mixed %s" % kw)
        assert got["status"][[1, 2, 4]].tolist() == [1, 1, 1]
        assert got["clique_size"][[1, 2]].tolist() == [0, 1] and got["clique_size"][4] <= 2
        assert np.array_equal(got["transform"][[1, 2, 4]], np.tile(np.eye(4), (3, 1, 1)))
        assert (got["iterations"][[1, 2, 4]] == 0).all()
        if kw:
            # every slot taken: the NaN point reaches the TIMs
            assert got["status"][6] == 2 and got["iterations"][6] == 1
            assert np.array_equal(got["transform"][6], np.eye(4)) and got["num_inliers"][6] == 0
        else:
            # the NaN point is an isolated vertex; the one-point target joins nothing
            assert got["status"][6] == 0 and 7 not in got["clique"][6]
            assert got["status"][7] == 1
            assert got["status"][5] == 1 and got["clique_size"][5] < 3  # every match wrong
        good = [0, 3, 8]
        alone = run(dev, x1[good], x2[good], i1[good], i2[good], count[good], **kw)
        for k in tr.KEYS:
            assert alone[k].tobytes() == got[k][good].tobytes(), k
        assert (got["status"][good] == 0).all()


def test_deterministic_and_batch_independent(dev):
    for name in ("m130", "noisy", "all_slots"):
        batch, kw, exp, gap = case(name)
        one, two = run(dev, *batch[:5], **kw), run(dev, *batch[:5], **kw)
        for k in tr.KEYS:
            assert one[k].tobytes() == two[k].tobytes(), (name, k)
        for q in range(len(batch[4])):
            alone = run(dev, *(a[q:q + 1] for a in batch[:5]), **kw)
            for k in tr.KEYS:
                assert alone[k][0].tobytes() == one[k][q].tobytes(), (name, q, k)


def test_argument_checks(dev):
    from pcr_amd import ops
    batch, kw, exp, gap = case("m130")
    t = [T(a, dev) for a in batch[:5]]
    for i, bad in ((0, t[0].double()), (0, t[0][:1]), (1, t[1][:, :2]), (2, t[2].long()),
                   (3, t[3][:, :100]), (4, t[4][:1]), (2, t[2].cpu())):
        args = list(t)
        args[i] = bad
        with pytest.raises(RuntimeError):
            ops.teaser(*args)
    for bad in (dict(noise_bound=0.0), dict(cbar2=-1.0), dict(gnc_factor=1.0), dict(max_iters=0),
                dict(max_iters=1001), dict(cost_threshold=-1.0), dict(seeds=-1)):
        with pytest.raises(RuntimeError, match="teaser"):
            ops.teaser(*t, **bad)
    big = torch.zeros((1, 3, 4097), device=dev)
    idx = torch.zeros((1, 4097), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="4096"):
        ops.teaser(big, big, idx, idx, idx[:, 0].contiguous())
    small = torch.empty(256, dtype=torch.uint8, device=dev)
    out = ops.teaser(*t, workspace=small, **kw)  # too small a workspace is replaced
    torch.cuda.synchronize()
    assert np.array_equal(N(out[1]), exp["clique"])


def test_side_stream_overwrites_poisoned_outputs(dev):
    """the C ABI on a stream of its own, into buffers pre-filled with garbage"""
    from pcr_amd import _lib
    for name in ("m130", "all_slots"):
        batch, kw, exp, gap = case(name)
        ref = run(dev, *batch[:5], **kw)
        t = [T(a, dev) for a in batch[:5]]
        p, n1, n2 = batch[0].shape[0], batch[0].shape[2], batch[1].shape[2]
        i32 = dict(dtype=torch.int32, device=dev)
        bufs = dict(transform=torch.full((p, 4, 4), float("nan"), dtype=torch.float64, device=dev),
                    clique=torch.full((p, n1), -77, **i32), inliers=torch.full((p, n1), -77, **i32),
                    **{k: torch.full((p,), -77, **i32)
                       for k in ("clique_size", "num_inliers", "iterations", "status")})
        lib = _lib.load()
        ws = torch.full((lib.pcr_teaser_workspace_size(p, n1),), 0xFF, dtype=torch.uint8,
                        device=dev)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        a = dict(tr.DEFAULTS, **kw)
        _lib.check(lib.pcr_teaser(
            *[x.data_ptr() for x in t[:2]], p, n1, n2, *[x.data_ptr() for x in t[2:]],
            a["noise_bound"], a["cbar2"], a["gnc_factor"], a["max_iters"], a["cost_threshold"],
            a["seeds"], int(a["inlier_selection"]), *[bufs[k].data_ptr() for k in tr.KEYS],
            ws.data_ptr(), ws.numel(), side.cuda_stream), "teaser")
        side.synchronize()
        for k in tr.KEYS:
            assert N(bufs[k]).tobytes() == ref[k].tobytes(), (name, k)


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
    x1, x2, gt, f1, f2, idx1, idx2 = feature_pairs(340, p, n, 32, 0.55)
    count = np.full(p, n, np.int32)
    exp, gap = tr.order_gap(x1, x2, idx1, idx2, count)
    iexp = ir.icp(x1, x2, exp["transform"], max_dist=0.2, max_iters=200, rel_fitness=1e-6,
                  rel_rmse=1e-6)
    return (x1, x2, gt, f1, f2, idx1, idx2, count), exp, gap, iexp


def test_register_pairs_with_the_teaser_solver(dev):
    from pcr_amd import ops
    from pcr_amd.registration import register_pairs, teaser_pairs
    (x1, x2, gt, f1, f2, idx1, idx2, count), exp, gap, iexp = end_to_end_case()
    # the input conditions: no near-tie, and a restatement that itself reaches
    # the ground truth, alone and followed by the ICP
    assert gap <= 1e-11 and (exp["status"] == 0).all()
    assert np.abs(exp["transform"] - gt).max() <= 1e-5
    assert (iexp["status"] == 0).all() and np.abs(iexp["transform"] - gt).max() <= 1e-5
    tx1, tx2, tf1, tf2 = (T(a, dev) for a in (x1, x2, f1, f2))
    plain = teaser_pairs(tx1, tx2, tf1, tf2)
    named = register_pairs(tx1, tx2, tf1, tf2, solver="teaser")
    both = register_pairs(tx1, tx2, tf1, tf2, solver="teaser", icp={})
    torch.cuda.synchronize()
    keys = {"idx1", "idx2", "count", "transform", "clique", "clique_size", "inliers",
            "num_inliers", "iterations", "reg_status"}
    assert set(plain) == set(named) == keys
    assert set(both) == keys | {"icp_" + k for k in ir.KEYS}
    for k, v in plain.items():
        assert N(both[k]).tobytes() == N(v).tobytes() == N(named[k]).tobytes(), k
    assert np.array_equal(N(plain["idx1"]), idx1) and np.array_equal(N(plain["idx2"]), idx2)
    assert np.array_equal(N(plain["count"]), count)
    # the solver is ops.teaser on the matching's output
    direct = ops.teaser(tx1, tx2, plain["idx1"], plain["idx2"], plain["count"])
    names = ("transform", "clique", "clique_size", "inliers", "num_inliers", "iterations",
             "reg_status")
    for k, v in zip(names, direct):
        assert N(plain[k]).tobytes() == N(v).tobytes(), k
    got = {k: N(plain["reg_status" if k == "status" else k]) for k in tr.KEYS}
    assert_matches(got, exp, "end to end")
    err = np.abs(got["transform"] - gt).max()
    print("end to end: %.3g from the ground truth" % err)
    assert err <= 1e-5
    # the refinement is ops.icp from the solver's transform, and stays at the ground truth
    refined = ops.icp(tx1, tx2, plain["transform"])
    for k, v in zip(ir.KEYS, refined):
        assert N(both["icp_" + k]).tobytes() == N(v).tobytes(), k
    err = np.abs(N(both["icp_transform"]) - gt).max()
    print("end to end: after ICP %.3g" % err)
    assert (N(both["icp_status"]) == 0).all() and err <= 1e-5
    # keywords reach the solver
    capped = register_pairs(tx1, tx2, tf1, tf2, solver="teaser", seeds=1, max_iters=7)
    direct = ops.teaser(tx1, tx2, plain["idx1"], plain["idx2"], plain["count"], seeds=1,
                        max_iters=7)
    for k, v in zip(names, direct):
        assert N(capped[k]).tobytes() == N(v).tobytes(), k


def test_the_other_solvers_are_what_they_were(dev):
    """solver="ransac" (the default) and solver="fgr" return ops.rigid_ransac /
    ops.fgr on the matching, with the keys they had"""
    from pcr_amd import ops
    from pcr_amd.registration import register_pairs
    (x1, x2, gt, f1, f2, idx1, idx2, count), _, _, _ = end_to_end_case()
    tx1, tx2, tf1, tf2 = (T(a, dev) for a in (x1, x2, f1, f2))
    kw = dict(hyps=256, inlier_dist=0.02, seed=3)
    default = register_pairs(tx1, tx2, tf1, tf2, **kw)
    named = register_pairs(tx1, tx2, tf1, tf2, solver="ransac", **kw)
    ransac = ops.rigid_ransac(tx1, tx2, default["idx1"], default["idx2"], default["count"], **kw)
    assert list(default) == list(named) == ["idx1", "idx2", "count", "transform", "inliers",
                                            "num_inliers", "best_hyp", "reg_status"]
    for k, v in zip(("transform", "inliers", "num_inliers", "best_hyp", "reg_status"), ransac):
        assert N(default[k]).tobytes() == N(v).tobytes() == N(named[k]).tobytes(), k
    fgr = register_pairs(tx1, tx2, tf1, tf2, solver="fgr", max_tuples=100)
    direct = ops.fgr(tx1, tx2, fgr["idx1"], fgr["idx2"], fgr["count"], max_tuples=100)
    assert list(fgr) == ["idx1", "idx2", "count", "transform", "slots", "num_corr", "num_trials",
                         "mu", "reg_status"]
    for k, v in zip(("transform", "slots", "num_corr", "num_trials", "mu", "reg_status"), direct):
        assert N(fgr[k]).tobytes() == N(v).tobytes(), k
    with pytest.raises(RuntimeError, match="unknown solver"):
        register_pairs(tx1, tx2, tf1, tf2, solver="teaserpp")


def test_pair_extractor_register_with_the_teaser_solver(dev):
    """2 pairs x 256 points through the extractor: the target is the source
    turned by 2 degrees and permuted, which already sends the matching of the
    extracted features wrong on 11 % of the first pair's correspondences and
    55 % of the second's; the solver equals the restatement on that matching
    and reaches the ground truth, and so does the ICP behind it"""
    from clouds import gaussian_clouds
    from pcr_amd import ops
    from pcr_amd.registration import PairExtractor
    p, n, c, k, r = 2, 256, 32, 16, 8
    xyz, nrm, feat = gaussian_clouds(2 * p, n, seed=49, c=c)
    rng = np.random.default_rng(p)
    gt = np.tile(np.eye(4), (p, 1, 1))
    truth = np.empty((p, n), np.int64)  # the target of source point i
    for i in range(p):
        rot = ir.rotation(rng, 2.0)
        perm = rng.permutation(n)
        xyz[p + i] = (rot @ xyz[i])[:, perm]
        nrm[p + i] = (rot @ nrm[i])[:, perm]
        feat[p + i] = feat[i][:, perm]
        gt[i, :3, :3] = rot
        truth[i, perm] = np.arange(n)
    xyz, nrm, feat = (a.astype(np.float32) for a in (xyz, nrm, feat))
    tx, tn, tf = (T(a, dev) for a in (xyz, nrm, feat))
    pe = PairExtractor(p, n, c, k, r, device=dev)
    out = pe.register(tx, tn, tf, solver="teaser", icp=dict(max_dist=0.1, max_iters=30), seeds=64)
    torch.cuda.synchronize()
    names = ("transform", "clique", "clique_size", "inliers", "num_inliers", "iterations",
             "reg_status")
    assert set(names) | {"icp_transform", "devox", "idx1"} <= set(out)
    direct = ops.teaser(tx[:p], tx[p:], out["idx1"], out["idx2"], out["count"], seeds=64)
    for key, v in zip(names, direct):
        assert N(out[key]).tobytes() == N(v).tobytes(), key
    count, i1, i2 = N(out["count"]), N(out["idx1"]), N(out["idx2"])
    wrong = []
    for q in range(p):
        m = int(count[q])
        wrong.append(float((truth[q, i1[q, :m]] != i2[q, :m]).mean()))
        print("pair %d: %d correspondences, %.0f %% wrong; clique %d, inliers %d, status %d" % (
            q, m, 100 * wrong[q], int(N(out["clique_size"])[q]), int(N(out["num_inliers"])[q]),
            int(N(out["reg_status"])[q])))
    assert max(wrong) >= 0.5  # the matching is as bad as the solver is meant for
    exp, gap = tr.order_gap(xyz[:p], xyz[p:], i1, i2, count, seeds=64)
    assert gap <= 1e-11 and np.abs(exp["transform"] - gt).max() <= 1e-5
    got = {key: N(out["reg_status" if key == "status" else key]) for key in tr.KEYS}
    assert_matches(got, exp, "extractor pairs")
    err = np.abs(got["transform"] - gt).max()
    ierr = np.abs(N(out["icp_transform"]) - gt).max()
    print("extractor pairs: solver %.3g, after ICP %.3g from the ground truth" % (err, ierr))
    assert (got["status"] == 0).all() and (N(out["icp_status"]) == 0).all()
    assert err <= 1e-5 and ierr <= 1e-5
