"""GPU: pcr_rigid_ransac (csrc/rigid.hip) through ops.rigid_ransac and
pcr_amd.registration against the numpy restatement of its contract
(tests/rigid_restate.py).

Synthetic pairs (test_rigid_cpu.synthetic_pair): source points in the unit
ball, target = R a + t rounded to fp32, a fraction of the targets replaced by
uniform outliers; tau = 0.02, rho = 0.9.  Bounds:
  exact    scores, best_hyp, num_inliers, inliers equal the restatement, under
           the asserted input condition that no deciding residual lies within
           1e-5 of tau (the fp32 residual chain errs by < 1e-6 on O(1) data);
  recovery max |R - R_gt|, |t - t_gt| <= 1e-5: the fp32 rounding of the
           inputs (6e-8 relative) through a fit over >= 25 spread inliers;
  refit    transform within 1e-8 of the SVD Kabsch over the reported mask
           (two fp64 algorithms on O(1) data);
  band     with sigma = 0.004 noise counts may flip at the threshold: the
           reported score lies between the restatement's counts at tau -+ 1e-5.
"""
import functools

import numpy as np
import pytest
import torch

import rigid_restate as rr
from test_rigid_cpu import _rot, synthetic_pair

pytestmark = pytest.mark.gpu

TAU, RHO = 0.02, 0.9
KEYS = ("transform", "inliers", "num_inliers", "best_hyp", "status", "scores")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def batch(seed, n1, n2, ms, outliers, noise=0.0):
    rng = np.random.default_rng(seed)
    pairs = [synthetic_pair(rng, n1, n2, m, outliers, noise) for m in ms]
    x1, x2, i1, i2, gt = (np.stack([pr[k] for pr in pairs]) for k in range(5))
    return dict(xyz1=x1, xyz2=x2, idx1=i1, idx2=i2, count=np.array(ms, np.int32), gt=gt)


# name -> (seed, n1, n2, counts, hyps, outlier fraction, refine_iters)
CASES = {
    "m3_h8": (11, 10, 8, (3,), 8, 0.0, 1),
    "m3_h1": (12, 3, 5, (3,), 1, 0.0, 2),
    "m64_61": (13, 80, 90, (64, 61), 256, 0.5, 2),
    "m300": (14, 300, 310, (300, 300, 300), 512, 0.55, 2),
    "m1000_h100": (15, 1000, 1100, (1000,), 100, 0.55, 2),  # hyps: no multiple of 64
    "m6000": (16, 6000, 6000, (6000,), 64, 0.55, 1),        # six LDS chunks of 1024 slots
    "mixed": (17, 200, 210, (0, 2, 3, 200), 128, 0.5, 2),
}


@functools.lru_cache(maxsize=None)
def case(name):
    seed, n1, n2, ms, hyps, outl, refine = CASES[name]
    b = batch(seed, n1, n2, ms, outl)
    exp = rr.ransac(b["xyz1"], b["xyz2"], b["idx1"], b["idx2"], b["count"], hyps, TAU, RHO,
                    refine, seed)
    return b, exp, dict(hyps=hyps, inlier_dist=TAU, edge_ratio=RHO, refine_iters=refine, seed=seed)


def run(dev, b, **kw):
    from pcr_amd import ops
    out = ops.rigid_ransac(T(b["xyz1"], dev), T(b["xyz2"], dev), T(b["idx1"], dev),
                           T(b["idx2"], dev), T(b["count"], dev), return_scores=True, **kw)
    torch.cuda.synchronize()
    return dict(zip(KEYS, (N(o) for o in out)))


def assert_exact(got, exp):
    for k in ("status", "scores", "best_hyp", "num_inliers", "inliers"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["transform"].dtype == np.float64
    bottom = np.tile([0.0, 0.0, 0.0, 1.0], (len(exp["status"]), 1))
    assert np.array_equal(got["transform"][:, 3], bottom)


def refit_parity(b, got):
    """max | transform - Kabsch over the reported mask | over the ok pairs"""
    worst = 0.0
    for q in np.nonzero((got["status"] == 0) & (got["num_inliers"] >= 3))[0]:
        m = got["inliers"][q].astype(bool)
        a = b["xyz1"][q][:, b["idx1"][q][m]].T
        c = b["xyz2"][q][:, b["idx2"][q][m]].T
        r, t = rr.kabsch(a, c)
        worst = max(worst, np.abs(got["transform"][q, :3, :3] - r).max(),
                    np.abs(got["transform"][q, :3, 3] - t).max())
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(dev, name):
    b, exp, kw = case(name)
    assert exp["margin"] > 1e-5  # the input condition of the exact comparison
    got = run(dev, b, **kw)
    assert_exact(got, exp)
    ok = exp["status"] == 0
    assert np.abs(got["transform"][~ok] - np.eye(4)).max(initial=0.0) == 0.0
    assert (got["best_hyp"][~ok] == -1).all() and (got["num_inliers"][~ok] == 0).all()
    par = refit_parity(b, got)
    print("%s: refit parity %.3g, against the restatement %.3g" % (
        name, par, np.abs(got["transform"] - exp["transform"]).max()))
    assert par <= 1e-8
    assert np.abs(got["transform"] - exp["transform"]).max() <= 1e-8
    big = ok & (b["count"] >= 60)
    if big.any():
        assert (got["num_inliers"][big] >= 25).all()
        err = np.abs(got["transform"][big] - b["gt"][big])
        print("%s: recovery R %.3g t %.3g" % (name, err[:, :3, :3].max(), err[:, :3, 3].max()))
        assert err[:, :3, :3].max() <= 1e-5
        assert np.linalg.norm(err[:, :3, 3], axis=1).max() <= 1e-5
    if name == "mixed":
        assert exp["status"].tolist() == [1, 1, 2, 0]  # the 3-slot pair holds an outlier
        assert (got["scores"][:2] == -1).all()


def test_noisy_band(dev):
    seed, hyps = 21, 512
    b = batch(seed, 300, 310, (300, 300, 300), 0.55, noise=0.004)
    kw = dict(hyps=hyps, inlier_dist=TAU, edge_ratio=RHO, refine_iters=0, seed=seed)
    got = run(dev, b, **kw)
    args = (b["xyz1"], b["xyz2"], b["idx1"], b["idx2"], b["count"], hyps, TAU, RHO, 0, seed)
    lo, hi = rr.ransac(*args, shift=-1e-5), rr.ransac(*args, shift=1e-5)
    assert (got["status"] == 0).all()
    for q in range(3):
        bh, sc = got["best_hyp"][q], got["scores"][q]
        assert bh >= 0 and sc[bh] == sc.max()
        assert lo["scores"][q][bh] <= sc[bh] <= hi["scores"][q][bh]
        assert lo["scores"][q].max() <= hi["scores"][q][bh]
        # the edge check is exact: the same hypotheses are rejected
        assert np.array_equal(sc < 0, lo["scores"][q] < 0)
        assert (lo["scores"][q] <= sc).all() and (sc <= hi["scores"][q]).all()
        # refine_iters = 0: the reported count is the best hypothesis' score
        assert got["num_inliers"][q] == sc[bh] == got["inliers"][q].sum()


def test_status_handling(dev):
    b, exp, kw = case("m64_61")
    # every target scaled by 3: no edge passes rho = 0.9
    scaled = dict(b, xyz2=(b["xyz2"] * np.float32(3.0)))
    got = run(dev, scaled, **kw)
    assert (got["status"] == 2).all() and (got["scores"] == -1).all()
    assert (got["best_hyp"] == -1).all() and (got["num_inliers"] == 0).all()
    assert (got["inliers"] == 0).all()
    assert np.array_equal(got["transform"], np.tile(np.eye(4), (2, 1, 1)))
    # rho = 0: nothing is rejected
    kw0 = dict(kw, edge_ratio=0.0)
    got = run(dev, b, **kw0)
    exp0 = rr.ransac(b["xyz1"], b["xyz2"], b["idx1"], b["idx2"], b["count"], kw["hyps"], TAU, 0.0,
                     kw["refine_iters"], kw["seed"])
    assert exp0["margin"] > 1e-5
    assert (got["scores"] >= 0).all()
    assert_exact(got, exp0)
    # without the optional scores the other outputs are the same
    from pcr_amd import ops
    dev_in = [T(b[k], dev) for k in ("xyz1", "xyz2", "idx1", "idx2", "count")]
    plain = ops.rigid_ransac(*dev_in, **kw0)
    assert len(plain) == 5
    for k, o in zip(KEYS, plain):
        assert np.array_equal(N(o), got[k]), k


def test_deterministic_and_seeded(dev):
    b, exp, kw = case("m64_61")
    one, two = run(dev, b, **kw), run(dev, b, **kw)
    for k in KEYS:
        assert one[k].tobytes() == two[k].tobytes(), k
    # every all-inlier triple scores the same: another seed meets its first one
    # at another h, and lands on the same transform
    other = run(dev, b, **dict(kw, seed=kw["seed"] + 1))
    assert (other["status"] == 0).all()
    assert (other["best_hyp"] != one["best_hyp"]).all()
    assert np.array_equal(other["num_inliers"], one["num_inliers"])
    assert np.abs(other["transform"] - one["transform"]).max() <= 1e-5


@pytest.mark.parametrize("channel_major", [False, True])
def test_register_pairs_end_to_end(dev, channel_major):
    from pcr_amd.registration import apply_transform, register_pairs, rre_rte
    p, n, c = 2, 300, 32
    rng = np.random.default_rng(31)
    b = batch(31, n, n, (n,) * p, 0.0)
    xyz1 = b["xyz1"]
    feat1 = rng.standard_normal((p, n, c)).astype(np.float32)
    xyz2, feat2, gt = np.empty_like(xyz1), np.empty_like(feat1), np.tile(np.eye(4), (p, 1, 1))
    for q in range(p):
        perm = rng.permutation(n)
        r, t = _rot(rng), rng.uniform(-0.5, 0.5, 3)
        gt[q, :3, :3], gt[q, :3, 3] = r, t
        xyz2[q] = (r @ xyz1[q].astype(np.float64) + t[:, None])[:, perm]
        feat2[q] = feat1[q][perm]
        noise = rng.permutation(n)[:int(0.4 * n)]
        feat2[q][noise] = rng.standard_normal((len(noise), c))
    if channel_major:
        feat1, feat2 = (np.ascontiguousarray(f.transpose(0, 2, 1)) for f in (feat1, feat2))
    tx1, tx2 = T(xyz1, dev), T(xyz2, dev)
    out = register_pairs(tx1, tx2, T(feat1, dev), T(feat2, dev), channel_major=channel_major,
                         hyps=256, inlier_dist=TAU, edge_ratio=RHO, refine_iters=2, seed=3)
    torch.cuda.synchronize()
    assert (N(out["reg_status"]) == 0).all()
    assert (N(out["count"]) >= 0.5 * n).all()
    assert (N(out["num_inliers"]) >= 0.5 * n).all()
    est = N(out["transform"])
    assert np.abs(est[:, :3, :3] - gt[:, :3, :3]).max() <= 1e-5
    assert np.linalg.norm(est[:, :3, 3] - gt[:, :3, 3], axis=1).max() <= 1e-5
    rre, rte = rre_rte(T(gt, dev), out["transform"])
    assert rre.max().item() < 0.1 and rte.max().item() < 1e-5
    moved = N(apply_transform(tx1, out["transform"]))
    # the inlier correspondences land on their targets (fp32 rounding of xyz2)
    for q in range(p):
        m = N(out["inliers"])[q].astype(bool)
        i1, i2 = N(out["idx1"])[q][m], N(out["idx2"])[q][m]
        assert np.abs(moved[q][:, i1] - xyz2[q][:, i2]).max() <= 1e-5


def test_pair_extractor_register(dev):
    from clouds import gaussian_clouds
    from pcr_amd import ops
    from pcr_amd.registration import PairExtractor
    p, n, c, k, r = 3, 1024, 32, 16, 16
    xyz, nrm, feat = gaussian_clouds(2 * p, n, seed=43, c=c)
    rng = np.random.default_rng(p)
    rot = _rot(rng)
    for i in range(p):
        perm = rng.permutation(n)
        xyz[p + i] = (rot @ xyz[i])[:, perm]
        nrm[p + i] = (rot @ nrm[i])[:, perm]
        feat[p + i] = feat[i][:, perm]
    tx, tn, tf = (T(a.astype(np.float32), dev) for a in (xyz, nrm, feat))
    pe = PairExtractor(p, n, c, k, r, device=dev)
    fwd = {key: v.clone() for key, v in pe.forward(tx, tn, tf).items()}
    kw = dict(hyps=128, inlier_dist=0.08, edge_ratio=RHO, refine_iters=2, seed=9)
    out = pe.register(tx, tn, tf, **kw)
    torch.cuda.synchronize()
    assert set(out) == set(fwd) | {"transform", "inliers", "num_inliers", "best_hyp", "reg_status"}
    for key, v in fwd.items():
        assert N(out[key]).tobytes() == N(v).tobytes(), key
    direct = ops.rigid_ransac(tx[:p], tx[p:], out["idx1"], out["idx2"], out["count"], **kw)
    for key, v in zip(("transform", "inliers", "num_inliers", "best_hyp", "reg_status"), direct):
        assert N(out[key]).tobytes() == N(v).tobytes(), key
    assert tuple(out["transform"].shape) == (p, 4, 4) and out["transform"].dtype == torch.float64
