"""CPU: the oracle restatements of SURVEY.md 8f rows f2 (LRF change_coords,
models/pvcnn_classify.py:153-184) and f4 (PointNet++ ops, sampling.cu,
neighbor_interpolate.cu), checked against independent PyTorch/NumPy
restatements of the reference's code.  The reference itself cannot run here
(SURVEY.md 8c), so these pins are "parity unpinned" against genuine reference
output.  The oracle is the checker of the GPU tests
(tests/test_gpu_pointnet2_lrf.py, tests/test_gpu_pointnet2_lrf_edges.py).

The second half checks the oracle against the float64 restatements of
tests/pointnet2_restate.py on every input family of the edges module.
Measured against float64, with a tolerance of 1e-5: three-NN weights off by at
most 1.1e-7 and interpolated features by 3.9e-7 (generic shapes, m = 0 .. 5,
lattice ties, far centres, NaN / Inf points and centres), no ambiguous point
skipped on any family (0 %); change_coords outputs off by at most 3.9e-7 on
the constructions clear of the thresholds and 1.7e-7 on the generic sizes,
no cloud left undecided; every furthest-point pick at exactly the float64
maximum (ratio 1.000000000)."""
import numpy as np
import pytest
import torch

import oracle
import pointnet2_restate as R
import sumorder
from clouds import gaussian_clouds


@pytest.mark.parametrize("b,n", [(3, 1024), (2, 37), (1, 2048)])
def test_oracle_lrf_matches_torch_restatement(b, n):
    xyz, _, _ = gaussian_clouds(b, n, seed=n)
    xyz = xyz + np.float32(0.25)  # non-centred input: the block centres it
    out, basis, picks, status = oracle.lrf_change_coords(xyz)
    ref, ref_picks, ref_status, margin = R.lrf_f64(xyz)
    assert (margin >= R.LRF_MARGIN).all()
    assert (status == 0).all() and (ref_status == 0).all()
    assert np.array_equal(picks, ref_picks)
    assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    for q in range(b):  # orthonormal, right-handed
        assert np.allclose(basis[q] @ basis[q].T, np.eye(3), atol=1e-6)
        assert np.linalg.det(basis[q]) > 0.999


def test_oracle_lrf_rotation_invariance():
    """The frame turns with the cloud: new coords of R x equal those of x."""
    xyz, _, _ = gaussian_clouds(2, 700, seed=3)
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    rot = np.einsum("ij,bjn->bin", q, xyz.astype(np.float64)).astype(np.float32)
    a, _, pa, _ = oracle.lrf_change_coords(xyz)
    r, _, pr, _ = oracle.lrf_change_coords(rot)
    assert np.array_equal(pa, pr)
    assert np.abs(a - r).max() < 1e-4


def test_oracle_lrf_asserts():
    # all points at the centroid: base_x has norm 0 (:159)
    z = np.zeros((1, 3, 16), np.float32)
    assert oracle.lrf_change_coords(z)[3][0] == 1
    # collinear cloud: no base_y with |lambda| < 0.9 (:169)
    t = np.linspace(-1, 1, 33, dtype=np.float32)
    line = np.stack([t, 2 * t, -t])[None]
    assert oracle.lrf_change_coords(line)[3][0] == 2


def test_oracle_fps_ties_follow_the_512_thread_reduction():
    """Every point at the same distance: the reference's reduction picks the
    lowest thread (k % 512) first, not the lowest index."""
    n = 1100
    # integer lattice points: every squared distance is exact, ties abound
    g = np.arange(n)
    xyz = np.stack([g % 11, (g // 11) % 10, g // 110]).astype(np.float32)[None]
    xyz[:, :, 512:] = xyz[:, :, :n - 512]  # k and k+512 coincide
    idx = oracle.furthest_point_sampling(xyz, 12)
    assert idx[0, 0] == 0
    assert np.array_equal(idx, R.fps_lattice_exact(xyz, 12))


def test_oracle_fps_matches_numpy_on_generic_clouds():
    xyz, _, _ = gaussian_clouds(2, 900, seed=7)
    idx = oracle.furthest_point_sampling(xyz, 64)
    for q in range(2):
        X = xyz[q].astype(np.float64)
        dist = np.full(900, np.inf)
        old, exp = 0, [0]
        for _ in range(63):
            dist = np.minimum(dist, ((X - X[:, old:old + 1]) ** 2).sum(0))
            old = int(np.argmax(dist))
            exp.append(old)
        assert idx[q].tolist() == exp


def test_oracle_three_nn_matches_numpy():
    rng = np.random.default_rng(2)
    b, n, m, c = 2, 300, 77, 5
    pts = rng.standard_normal((b, 3, n)).astype(np.float32)
    ctr = rng.standard_normal((b, 3, m)).astype(np.float32)
    cf = rng.standard_normal((b, c, m)).astype(np.float32)
    out, inds, wgts = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    for q in range(b):
        d = ((pts[q][:, :, None].astype(np.float64) - ctr[q][:, None, :]) ** 2).sum(0)
        order = np.argsort(d, axis=1, kind="stable")[:, :3]
        assert np.array_equal(inds[q].T, order)
        dd = np.maximum(np.take_along_axis(d, order, 1), 1e-10)
        w = (1.0 / dd) / (1.0 / dd).sum(1, keepdims=True)
        assert np.abs(wgts[q].T - w).max() < 1e-5
        ref = np.einsum("cnk,nk->cn", cf[q][:, order], w)
        assert np.abs(out[q] - ref).max() < 1e-5
    g = rng.standard_normal((b, c, n)).astype(np.float32)
    gx = oracle.three_nearest_neighbors_interpolate_backward(g, inds, wgts, m)
    exp = np.zeros((b, c, m))
    for q in range(b):
        for a in range(3):
            np.add.at(exp[q].T, inds[q, a], (g[q] * wgts[q, a]).T)
    assert np.abs(gx - exp).max() < 1e-5


def test_oracle_three_nn_fewer_than_three_centres():
    pts = np.zeros((1, 3, 4), np.float32)
    ctr = np.ones((1, 3, 2), np.float32)
    cf = np.array([[[1.0, 3.0]]], np.float32)
    out, inds, wgts = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    assert inds[0, :, 0].tolist() == [0, 1, 0]  # unfilled slot keeps index 0
    assert abs(wgts[0, 2, 0]) < 1e-9          # 1e10 clamp -> negligible weight


def test_oracle_gather_roundtrip():
    rng = np.random.default_rng(4)
    f = rng.standard_normal((2, 4, 50)).astype(np.float32)
    idx = rng.integers(0, 50, (2, 30)).astype(np.int32)
    out = oracle.gather_features_forward(f, idx)
    assert np.array_equal(out, np.take_along_axis(f, idx[:, None, :].repeat(4, 1), 2))
    g = rng.standard_normal((2, 4, 30)).astype(np.float32)
    gx = oracle.gather_features_backward(g, idx, 50)
    exp = np.zeros((2, 4, 50), np.float32)
    for q in range(2):
        np.add.at(exp[q].T, idx[q], g[q].T)
    assert np.abs(gx - exp).max() < 1e-5


def test_losses_match_reference_formulas():
    import PVCNN.modules.functional as F
    torch.manual_seed(0)
    x, y = torch.randn(4, 6), torch.randn(4, 6)
    p = torch.softmax(x, 1)
    exp = torch.mean(torch.sum(p * (torch.log(p) - torch.log_softmax(y, 1)), 1))
    assert torch.allclose(F.kl_loss(x, y), exp)
    e = torch.randn(100) * 3
    q = torch.minimum(e.abs(), torch.full_like(e, 1.5))
    assert torch.allclose(F.huber_loss(e, 1.5), torch.mean(0.5 * q ** 2 + 1.5 * (e.abs() - q)))


# ---------------------------------------------------------------------------
# The oracle on every input family of test_gpu_pointnet2_lrf_edges.py against
# the float64 restatements of pointnet2_restate.py, which share no code with
# include/pcr_math.h.
def _three_nn_vs_f64(pts, ctr, cf, exact=False):
    out, inds, wgts = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    fig = R.check_three_nn(out, inds, wgts, R.three_nn_f64(pts, ctr, cf), exact=exact)
    print("skipped %.4f%%, weights %.3g, out %.3g" % (100 * fig[0], fig[1], fig[2]))
    return out, inds, wgts, fig


@pytest.mark.parametrize("n,m", R.NN_GENERIC)
def test_oracle_three_nn_generic_vs_f64(n, m):
    pts, ctr, cf = R.nn_generic(n, m)
    fig = _three_nn_vs_f64(pts, ctr, cf)[3]
    assert fig[0] == 0.0  # no ambiguous point at these shapes and seeds


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4, 5])
def test_oracle_three_nn_few_centres_vs_f64(m):
    """Unfilled slots keep index 0 and the 1e10 clamp; m = 0 gives zeros and
    weights 1/3."""
    pts, ctr, cf = R.nn_generic(257, m, c=3)
    out, inds, wgts, _ = _three_nn_vs_f64(pts, ctr, cf)
    if m == 0:
        assert (out == 0).all() and (inds == 0).all()
        assert np.abs(wgts - 1.0 / 3.0).max() < 1e-7


def test_oracle_three_nn_ties_are_exact():
    """Integer lattice: nothing is skipped, the stable argsort is the answer,
    and the planted ties resolve to the lower index."""
    pts, ctr, expected = R.nn_tie_centres()
    cf = R.features_for(ctr, 5)
    out, inds, wgts, fig = _three_nn_vs_f64(pts, ctr, cf, exact=True)
    assert fig[0] == 0.0
    for j, triple in expected.items():
        assert tuple(inds[0, :, j]) == triple
    on_centre = [j for j in expected if j % 3 == 2]  # d = 0: the 1e-10 clamp
    assert len(on_centre) == 4 and (wgts[0, 0, on_centre] == 1).all()
    w1 = wgts[0, 1, on_centre].astype(np.float64)  # (1 / 4) / (1 / 1e-10)
    assert np.abs(w1 / 2.5e-11 - 1.0).max() < 1e-6


def test_oracle_three_nn_far_centres_meet_the_clamp():
    pts, ctr = R.nn_far_centres()
    cf = R.features_for(ctr, 5)
    out, inds, wgts, _ = _three_nn_vs_f64(pts, ctr, cf)
    assert (inds[:, 0] == 2).all() and (inds[:, 1:] != 2).all()
    assert np.array_equal(wgts[:, 1], wgts[:, 2])  # both clamped to 1e10
    assert (wgts[:, 1] > 0).all() and wgts[:, 1].max() < 1e-8


@pytest.mark.parametrize("case", [0, 1])
def test_oracle_three_nn_special_values(case):
    """A NaN or infinite distance never enters: such a query keeps index 0
    three times with weights 1/3, such a centre is never chosen."""
    name, pts, ctr = R.nn_special_cases()[case]
    cf = R.features_for(ctr, 5)
    out, inds, wgts, _ = _three_nn_vs_f64(pts, ctr, cf)
    assert np.isfinite(wgts).all() and np.isfinite(out).all()
    if name == "points":
        for q, j in ((0, 7), (1, 290), (2, 7), (2, 290)):
            assert inds[q, :, j].tolist() == [0, 0, 0]
    else:
        assert not (inds[0] == 6).any() and not (inds[1] == 1026).any()
        assert not np.isin(inds[2], (6, 1026)).any()


def _scatter_f64(ids, terms, size):
    """sum of terms [c, k] per target, float64; ids outside [0, size) drop."""
    ok = (ids >= 0) & (ids < size)
    return np.stack([np.bincount(ids[ok], weights=t[ok], minlength=size) for t in terms])


@pytest.mark.parametrize("hub", [False, True])
def test_oracle_three_nn_backward_vs_f64(hub):
    """The forward's own indices and weights with guard slots planted (-1, m,
    m + 5 are dropped), and a hub (m = 8 centres, 4096 points)."""
    n, m, c = (4096, 8, 5) if hub else (700, 1027, 5)
    pts, ctr, cf = R.nn_generic(n, m, c)
    _, inds, wgts = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    inds = inds.copy()
    inds[:, 0, 3], inds[:, 1, 4], inds[:, 2, n - 1] = -1, m, m + 5
    g = np.random.default_rng(n).standard_normal((2, c, n)).astype(np.float32)
    gx = oracle.three_nearest_neighbors_interpolate_backward(g, inds, wgts, m)
    bound = sumorder.three_nn_backward_bound(g, inds, wgts, m)
    exp = np.zeros((2, c, m))
    for q in range(2):
        for a in range(3):
            t = (wgts[q, a][None, :] * g[q]).astype(np.float32).astype(np.float64)
            exp[q] += _scatter_f64(inds[q, a].astype(np.int64), t, m)
    sumorder.assert_within_sum_order(gx, exp, bound)
    if hub:
        assert np.bincount(inds[inds >= 0].ravel(), minlength=m + 6)[:m].max() > 2000


def test_oracle_gather_guards_and_hub_vs_f64():
    rng = np.random.default_rng(6)
    b, c, n, m = 2, 7, 50, 3000
    f = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    idx[1] = 17                                        # every j maps to one index
    idx[:, 5], idx[:, 6], idx[:, m - 1] = -1, n, n + 5
    out = oracle.gather_features_forward(f, idx)
    ok = (idx >= 0) & (idx < n)
    exp = np.where(ok[:, None, :], np.take_along_axis(f, np.clip(idx, 0, n - 1)[:, None, :]
                                                      .repeat(c, 1), 2), np.float32(0))
    assert np.array_equal(out, exp) and not np.signbit(out[:, :, 5]).any()
    g = rng.standard_normal((b, c, m)).astype(np.float32)
    gx = oracle.gather_features_backward(g, idx, n)
    ref = np.stack([_scatter_f64(idx[q].astype(np.int64), g[q].astype(np.float64), n)
                    for q in range(b)])
    sumorder.assert_within_sum_order(gx, ref, sumorder.gather_backward_bound(g, idx, n))
    assert (gx[1, :, :17] == 0).all() and (gx[1, :, 18:] == 0).all()


def test_backward_bounds_count_terms():
    """One term: bound 0 (bit-exact).  k equal terms: 2 gamma(k - 1) k |t|."""
    g = np.ones((1, 1, 4), np.float32)
    idx = np.array([[0, 2, 2, 9]], np.int32)
    bnd = sumorder.gather_backward_bound(g, idx, 3)
    assert bnd[0, 0].tolist() == [0.0, 0.0, 2 * float(sumorder.gamma(1)) * 2]
    inds = np.array([[[0, 1, 1, 1], [1, -1, 3, 1], [2, 2, 2, 2]]], np.int32)
    w = np.full((1, 3, 4), 0.5, np.float32)
    bnd = sumorder.three_nn_backward_bound(g, inds, w, 3)
    assert np.allclose(bnd[0, 0], [0.0, 2 * sumorder.gamma(4) * 2.5, 2 * sumorder.gamma(3) * 2.0])


@pytest.mark.parametrize("n", R.FPS_LINES + (40, 5, 1))
def test_oracle_fps_is_greedy_at_the_dispatch_sizes(n):
    xyz = R.fps_generic(2, n)
    idx = oracle.furthest_point_sampling(xyz, 8)
    worst = R.fps_greedy_check(xyz, idx)
    print("smallest dist[pick] / max(dist): %.9f" % worst)
    assert idx.shape == (2, 8) and (idx[:, 0] == 0).all()
    if n == 1:
        assert (idx == 0).all()
    assert oracle.furthest_point_sampling(xyz, 1).tolist() == [[0], [0]]


@pytest.mark.parametrize("duplicate", [True, False])
@pytest.mark.parametrize("n", [40, 600, 1100, 9000])
def test_oracle_fps_lattice_vs_exact_rule(n, duplicate):
    xyz = R.lattice_cloud(n, duplicate)
    exp = R.fps_lattice_exact(xyz, 40)
    assert np.array_equal(oracle.furthest_point_sampling(xyz, 40), exp)
    if n > 512 and not duplicate:  # the rule is not "the lowest index" here
        X, low = xyz.astype(np.float64), np.zeros_like(exp)
        for q in range(2):
            dist = np.full(n, np.inf)
            for j in range(1, 40):
                dist = np.minimum(dist, ((X[q] - X[q][:, low[q, j - 1], None]) ** 2).sum(axis=0))
                low[q, j] = np.argmax(dist)
        assert (low != exp).any()


def test_oracle_fps_coincident_cloud():
    xyz = np.full((2, 3, 700), 1.25, np.float32)
    idx = oracle.furthest_point_sampling(xyz, 9)
    assert (idx == 0).all() and np.array_equal(idx, R.fps_lattice_exact(xyz, 9))


@pytest.mark.parametrize("n", sorted(R.FPS_SPECIAL))
def test_oracle_fps_special_values(n):
    xyz = R.special_clouds(n, *R.FPS_SPECIAL[n])
    assert np.array_equal(oracle.furthest_point_sampling(xyz, 6), R.fps_special_expected(n, 6))


@pytest.mark.parametrize("name", sorted(R.LRF_EDGES))
def test_oracle_lrf_threshold_edges(name):
    """One float on either side of lambda = +-0.9 and of the 1e-5 norms.  The
    expectations follow from fp32 arithmetic restated in numpy
    (R.f32_lambda), not from the oracle.  Status 3 is out of reach: once
    |lambda| < 0.9 the Gram-Schmidt remainder has norm sqrt(1 - lambda^2) >
    0.43."""
    xyz, status, picks = R.LRF_EDGES[name]
    if name.startswith("lambda"):
        lam = R.f32_lambda(*xyz[0, :, 2])
        side = {"inside": R.below(R.LAM), "on": R.LAM, "outside": R.above(R.LAM)}
        assert abs(lam) == side[name.rsplit("-", 1)[1]] and (lam < 0) == (name[6] == "-")
    else:
        v = xyz[0, 1, -2]
        assert np.sqrt(v * v) == v  # the fp32 norm is the coordinate itself
    _, basis, got_picks, got_status = oracle.lrf_change_coords(xyz)
    assert got_status[0] == status and tuple(got_picks[0]) == picks
    if status == 0:
        assert np.allclose(basis[0] @ basis[0].T, np.eye(3), atol=1e-6)


def _lrf_vs_f64(xyz, exact_ties=False):
    """-> (undecided share, max |out - ref| / max(1, |ref|)) over the decided
    clouds."""
    out, _, picks, status = oracle.lrf_change_coords(xyz)
    ref, ref_picks, ref_status, margin = R.lrf_f64(xyz, exact_ties)
    use = margin >= R.LRF_MARGIN
    assert np.array_equal(status[use], ref_status[use])
    assert np.array_equal(picks[use], ref_picks[use])
    ok = use & (ref_status == 0)
    err = float((np.abs(out[ok] - ref[ok]) / max(1.0, np.abs(ref[ok]).max(initial=0))).max(initial=0))
    assert err <= R.TOL
    assert (out[status != 0] == 0).all()
    return 1.0 - use.mean(), err


@pytest.mark.parametrize("name", sorted(R.LRF_CLEAR))
def test_oracle_lrf_clear_of_thresholds_vs_f64(name):
    xyz, status, picks = R.LRF_CLEAR[name]
    _, _, got_picks, got_status = oracle.lrf_change_coords(xyz)
    assert got_status[0] == status and tuple(got_picks[0]) == picks
    undecided, err = _lrf_vs_f64(xyz, exact_ties=True)  # mirror pairs, mean exactly 0
    assert undecided == 0
    print("out %.3g" % err)


@pytest.mark.parametrize("b,n", R.LRF_SIZES)
def test_oracle_lrf_sizes_vs_f64(b, n):
    """n = 2: the centred points are mirror images, so whichever ranks first
    (rounding decides), the other has lambda = -1 and nothing qualifies."""
    if n == 2:
        out, basis, picks, status = oracle.lrf_change_coords(R.lrf_generic(b, n))
        assert (status == 2).all() and (picks[:, 1] == -1).all() and (picks[:, 0] >= 0).all()
        assert (out == 0).all() and (basis == 0).all()
        return
    undecided, err = _lrf_vs_f64(R.lrf_generic(b, n))
    print("undecided %.4f, out %.3g" % (undecided, err))
    assert undecided <= R.LRF_UNDECIDED_CAP


def test_oracle_lrf_special_values():
    """A NaN norm ranks first (torch.argsort, descending), so base_x fails its
    assert: status 1 for a NaN and for an infinite coordinate (the infinite
    mean turns that point's own norm into NaN)."""
    xyz = R.special_clouds(600, 520, 100)
    out, basis, picks, status = oracle.lrf_change_coords(xyz)
    assert status.tolist() == [1, 1, 1]
    assert picks.tolist() == [[0, -1], [100, -1], [0, -1]]
    assert (basis == 0).all() and np.isnan(out).any(axis=(1, 2)).all()
