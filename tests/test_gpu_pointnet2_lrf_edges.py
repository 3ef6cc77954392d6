"""The kernels of csrc/pointnet2.hip and csrc/lrf.hip where they can go wrong
unseen, bit for bit against the oracle and against the independent float64
restatements of tests/pointnet2_restate.py (test_pointnet2_lrf_cpu.py pins the
oracle on the same inputs):

 - three_nn_kernel: the scalar tail after a float4 body and in a later LDS
   tile, exact ties inside a float4 group, across groups and across the tile
   boundary, a four-way tie at the third place, both weight clamps, m = 0,
   channel counts ragged over the channel groups, NaN / Inf coordinates;
 - the grid-stride loops of the gathers and of three_nn_grad_kernel past
   65,536 blocks, their index guards (-1, the size, the size + 5), and hub
   targets under the per-element bound of tests/sumorder.py;
 - furthest point sampling on both sides of every dispatch line, m = 1,
   m > n, fewer points than a wave, an all-coincident cloud, NaN / Inf points
   on the register and on the streaming path;
 - change_coords one float on either side of lambda = +-0.9 and of the 1e-5
   norms, n = 2 .. 1025, 300 clouds in one launch, NaN / Inf clouds.

change_coords status 3 (the Gram-Schmidt assert) is not tested: it cannot be
reached.  Once |lambda| < 0.9 holds, the remainder of base_x has norm
sqrt(1 - lambda^2) > 0.43, far from 1e-5.

Every output buffer of the direct C calls is poisoned first."""
import functools

import numpy as np
import pytest

import oracle
import pointnet2_restate as R
import sumorder

pytestmark = pytest.mark.gpu


def T(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the cases are read-only


def N(t):
    return t.detach().cpu().numpy()


def assert_bits(got, exp, what):
    if np.array_equal(got, exp, equal_nan=got.dtype.kind == "f"):
        return
    bad = np.argwhere(~((got == exp) | ((got != got) & (exp != exp))))
    raise AssertionError("%s differs at %d of %d places, first %s: got %r exp %r" % (
        what, len(bad), got.size, bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])]))


# ------------------------------------------------------- three-NN forward
def run_three_nn(dev, pts, ctr, cf):
    """pcr_three_nn_interpolate_forward through the C ABI on poisoned outputs
    (empty inputs get a one-element buffer, never a null pointer)."""
    import torch
    from pcr_amd import _lib
    from pcr_amd.ops import _ptr, _stream
    b, c, m = cf.shape
    n = pts.shape[2]
    tp, tc, tf = (T(a, dev) if a.size else torch.zeros(1, device=dev) for a in (pts, ctr, cf))
    out = torch.full((b, c, n), float("nan"), device=dev)
    inds = torch.full((b, 3, n), -7, dtype=torch.int32, device=dev)
    wgts = torch.full((b, 3, n), float("nan"), device=dev)
    po = out if out.numel() else torch.zeros(1, device=dev)
    _lib.check(_lib.load().pcr_three_nn_interpolate_forward(
        _ptr(tp), _ptr(tc), _ptr(tf), b, c, m, n, _ptr(po), _ptr(inds), _ptr(wgts), _stream()),
        "three_nn_interpolate_forward")
    torch.cuda.synchronize()
    return N(out), N(inds), N(wgts)


def check_three_nn(dev, pts, ctr, cf, exact=False):
    got = run_three_nn(dev, pts, ctr, cf)
    exp = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    assert_bits(got[1], exp[1], "indices")
    assert_bits(got[2], exp[2], "weights")
    assert_bits(got[0], exp[0], "interpolated features")
    R.check_three_nn(*got, R.three_nn_f64(pts, ctr, cf), exact=exact)
    return got


@pytest.mark.parametrize("n,c", [(1, 1), (255, 15), (257, 17), (700, 65)])
@pytest.mark.parametrize("m", [3, 4, 5, 7, 1023, 1024, 1025, 1027, 2051, 0])
def test_three_nn_tails_and_channel_groups(dev, m, n, c):
    """m = 5, 7: a tail after a float4 body; 1023: a tail of 3 after 255
    groups; 1025, 1027, 2051: a tail in a later tile (1, 3, 3); 3: a tail
    only; 0: no centre (zeros, weights from the 1e10 clamp).  n = 255, 257
    and 700 end a block early; c = 15 is one channel group, 17 two (9 + 8), 65
    four (17, 17, 17, 14), 1 the smallest."""
    pts, ctr, cf = R.nn_generic(n, m, c)
    out, inds, wgts = check_three_nn(dev, pts, ctr, cf)
    if m == 0:
        assert (out == 0).all() and (inds == 0).all()
        assert np.abs(wgts - 1.0 / 3.0).max() < 1e-7


@pytest.mark.parametrize("c", [5, 17])
def test_three_nn_exact_ties(dev, c):
    """Integer lattice, nothing skipped: the lower index wins a tie inside a
    float4 group, across groups, across the tile boundary (float4 body and
    scalar tail), and a fourth equidistant centre never displaces the third.
    Queries on a centre meet the 1e-10 clamp."""
    pts, ctr, expected = R.nn_tie_centres()
    out, inds, wgts = check_three_nn(dev, pts, ctr, R.features_for(ctr, c), exact=True)
    for j, triple in expected.items():
        assert tuple(inds[0, :, j]) == triple, (j, inds[0, :, j], triple)


def test_three_nn_far_centres(dev):
    pts, ctr = R.nn_far_centres()
    out, inds, wgts = check_three_nn(dev, pts, ctr, R.features_for(ctr, 5))
    assert np.array_equal(wgts[:, 1], wgts[:, 2]) and (wgts[:, 1] > 0).all()


@pytest.mark.parametrize("case", [0, 1], ids=["points", "centres"])
def test_three_nn_special_values(dev, case):
    _, pts, ctr = R.nn_special_cases()[case]
    out, inds, wgts = check_three_nn(dev, pts, ctr, R.features_for(ctr, 17))
    assert np.isfinite(wgts).all() and np.isfinite(out).all()


# ------------------------------------------------------ three-NN backward
@functools.lru_cache(maxsize=None)
def nn_backward_case(n, m, c, guards):
    """-> (grad_y, inds, wgts, expected grad_x, bound), read-only: the
    oracle forward's own indices and weights, with `guards` three slots set to
    -1, m and m + 5."""
    pts, ctr, cf = R.nn_generic(n, m, c)
    _, inds, wgts = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, cf)
    if guards:
        inds[:, 0, 3], inds[:, 1, n // 2], inds[:, 2, n - 1] = -1, m, m + 5
    g = np.random.default_rng(n + m).standard_normal((2, c, n)).astype(np.float32)
    exp = oracle.three_nearest_neighbors_interpolate_backward(g, inds, wgts, m)
    return R._ro(g, inds, wgts, exp, sumorder.three_nn_backward_bound(g, inds, wgts, m))


@pytest.mark.parametrize("n,m,c,guards", [(700, 1027, 17, False), (700, 1027, 17, True),
                                          (4096, 8, 5, False)],
                         ids=["own", "guards", "hub"])
def test_three_nn_backward_within_sum_order(dev, n, m, c, guards):
    """The guard drops slots of -1, m and m + 5; with m = 8 and n = 4096 a
    centre receives thousands of terms per channel."""
    from pcr_amd import ops
    g, inds, wgts, exp, bound = nn_backward_case(n, m, c, guards)
    gx = ops.three_nearest_neighbors_interpolate_backward(T(g, dev), T(inds, dev), T(wgts, dev), m)
    sumorder.assert_within_sum_order(N(gx), exp, bound)
    if m == 8:
        assert np.bincount(inds.ravel(), minlength=m).max() > 2000


# ------------------------------------------------------------------ gather
def test_gather_guards_and_hub(dev):
    """Indices of -1, n and n + 5 read +0 forward and add nothing backward;
    cloud 1 maps every j to one index, which then sums 2997 terms."""
    from pcr_amd import ops
    rng = np.random.default_rng(6)
    b, c, n, m = 2, 7, 300, 3000
    f = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    idx[1] = 17
    idx[:, 5], idx[:, 6], idx[:, m - 1] = -1, n, n + 5
    out = N(ops.gather_features_forward(T(f, dev), T(idx, dev)))
    assert_bits(out, oracle.gather_features_forward(f, idx), "gather forward")
    assert (out[:, :, (5, 6, m - 1)] == 0).all() and not np.signbit(out[:, :, (5, 6, m - 1)]).any()
    g = rng.standard_normal((b, c, m)).astype(np.float32)
    gx = N(ops.gather_features_backward(T(g, dev), T(idx, dev), n))
    sumorder.assert_within_sum_order(gx, oracle.gather_features_backward(g, idx, n),
                                     sumorder.gather_backward_bound(g, idx, n))


# ------------------------------------------------------------- grid stride
STRIDE_C = 33  # 33 * 2^19 = 17,301,504 elements > 65,536 blocks * 256 threads


def test_gather_grid_stride(dev):
    """More elements than 65,536 blocks of 256 threads: the tensor's last
    524,288 elements are reached only by the second trip of the grid-stride
    loop.  n = 4096 keeps a target at about 128 terms, so the backward bound
    stays tight (1.5e-5 of the sum of the terms' magnitudes)."""
    from pcr_amd import ops
    rng = np.random.default_rng(8)
    n, m = 4096, 2 ** 19
    assert STRIDE_C * m > 65536 * 256
    f = rng.standard_normal((1, STRIDE_C, n), dtype=np.float32)
    idx = rng.integers(-1, n + 1, (1, m)).astype(np.int32)  # -1 and n included
    out = N(ops.gather_features_forward(T(f, dev), T(idx, dev)))
    assert_bits(out, oracle.gather_features_forward(f, idx), "gather forward")
    g = rng.standard_normal((1, STRIDE_C, m), dtype=np.float32)
    gx = N(ops.gather_features_backward(T(g, dev), T(idx, dev), n))
    sumorder.assert_within_sum_order(gx, oracle.gather_features_backward(g, idx, n),
                                     sumorder.gather_backward_bound(g, idx, n))


def test_three_nn_backward_grid_stride(dev):
    """The same element count over b * c * n with m = 8: 8192 clouds of 64
    points, so a centre sums about 20 terms and the bound stays tight; the
    last 248 clouds lie past the first trip of the loop."""
    from pcr_amd import ops
    rng = np.random.default_rng(9)
    b, n, m = 8192, 64, 8
    assert b * STRIDE_C * n > 65536 * 256
    inds = rng.integers(-1, m + 1, (b, 3, n)).astype(np.int32)  # -1 and m included
    wgts = rng.random((b, 3, n), dtype=np.float32)
    g = rng.standard_normal((b, STRIDE_C, n), dtype=np.float32)
    gx = N(ops.three_nearest_neighbors_interpolate_backward(T(g, dev), T(inds, dev),
                                                            T(wgts, dev), m))
    sumorder.assert_within_sum_order(
        gx, oracle.three_nearest_neighbors_interpolate_backward(g, inds, wgts, m),
        sumorder.three_nn_backward_bound(g, inds, wgts, m))


# --------------------------------------------------------------------- FPS
def run_fps(dev, xyz, m):
    import torch
    from pcr_amd import ops
    got = ops.furthest_point_sampling(T(xyz, dev), m)
    torch.cuda.synchronize()
    got = N(got)
    assert_bits(got, oracle.furthest_point_sampling(xyz, m), "picks")
    return got


@pytest.mark.parametrize("n", R.FPS_LINES)
def test_fps_dispatch_lines(dev, n):
    """fps_reg_kernel<1, 2, 4, 8, 16, 32> and fps_big_kernel, each from its
    smallest and to its largest n."""
    xyz = R.fps_generic(2, n)
    R.fps_greedy_check(xyz, run_fps(dev, xyz, 8))


@pytest.mark.parametrize("n,m", [(300, 1), (9000, 1), (1, 4), (5, 9), (40, 8), (40, 64)])
def test_fps_small_counts(dev, n, m):
    """m = 1 runs no step; m > n revisits points at distance 0; with n = 40
    three of the four waves hold no point and post the empty key."""
    xyz = R.fps_generic(2, n)
    R.fps_greedy_check(xyz, run_fps(dev, xyz, m))


@pytest.mark.parametrize("n", [40, 500, 600, 700, 9000])
def test_fps_lattice_and_coincident(dev, n):
    """Exact distances: the largest, then the lowest k % 512, then the lowest
    k (distinct lattice points: the rule differs from the lowest index once
    n > 512).  n = 700: every point in one place, every key ties at distance
    0."""
    xyz = np.full((2, 3, n), 1.25, np.float32) if n == 700 else R.lattice_cloud(n, False)
    got = run_fps(dev, xyz, 24)
    assert_bits(got, R.fps_lattice_exact(xyz, 24), "picks against the exact rule")
    if n == 700:
        assert (got == 0).all()


@pytest.mark.parametrize("n", sorted(R.FPS_SPECIAL))
def test_fps_special_values(dev, n):
    """fminf keeps the 1e38 of a NaN or infinite point: it is picked at step 1
    and at every step after (n = 600 in registers, 9000 streamed)."""
    xyz = R.special_clouds(n, *R.FPS_SPECIAL[n])
    assert_bits(run_fps(dev, xyz, 6), R.fps_special_expected(n, 6), "picks")


# --------------------------------------------------------------------- LRF
def run_lrf(dev, xyz):
    """-> (out, basis, picks, status), bit for bit the oracle's."""
    import torch
    from pcr_amd import ops
    out, (basis, picks, status) = ops.lrf_change_coords(T(xyz, dev), check=False,
                                                        return_basis=True)
    torch.cuda.synchronize()
    got = tuple(N(a) for a in (out, basis, picks, status))
    for g, e, what in zip(got, oracle.lrf_change_coords(xyz), ("out", "basis", "picks", "status")):
        assert_bits(g, e, what)
    return got


def lrf_against_f64(xyz, got, exact_ties=False):
    """The clouds that lrf_f64 can decide: same status and picks, outputs
    within 1e-5.  -> the undecided share."""
    out, _, picks, status = got
    ref, ref_picks, ref_status, margin = R.lrf_f64(xyz, exact_ties)
    use = margin >= R.LRF_MARGIN
    assert np.array_equal(status[use], ref_status[use])
    assert np.array_equal(picks[use], ref_picks[use])
    ok = use & (ref_status == 0)
    scale = max(1.0, np.abs(ref[ok]).max(initial=0))
    assert np.abs(out[ok] - ref[ok]).max(initial=0) <= R.TOL * scale
    return 1.0 - use.mean()


@pytest.mark.parametrize("name", sorted(R.LRF_EDGES))
def test_lrf_threshold_edges(dev, name):
    """lambda one float inside, on and outside +0.9 and -0.9; the norms of
    base_y and base_x one float below, on and above 1e-5."""
    xyz, status, picks = R.LRF_EDGES[name]
    got = run_lrf(dev, xyz)
    assert got[3][0] == status and tuple(got[2][0]) == picks


@pytest.mark.parametrize("name", sorted(R.LRF_CLEAR))
def test_lrf_clear_of_thresholds(dev, name):
    xyz, status, picks = R.LRF_CLEAR[name]
    got = run_lrf(dev, xyz)
    assert got[3][0] == status and tuple(got[2][0]) == picks
    assert lrf_against_f64(xyz, got, exact_ties=True) == 0


@pytest.mark.parametrize("b,n", R.LRF_SIZES)
def test_lrf_sizes(dev, b, n):
    """n = 2 (mirror images: status 2), 3, 63 and 65 (around a wave), 1025
    (one point past the 1024 threads), and 300 clouds of 64 points."""
    xyz = R.lrf_generic(b, n)
    got = run_lrf(dev, xyz)
    if n == 2:
        assert (got[3] == 2).all() and (got[0] == 0).all()
    else:
        assert lrf_against_f64(xyz, got) <= R.LRF_UNDECIDED_CAP


def test_lrf_special_values(dev):
    xyz = R.special_clouds(600, 520, 100)
    out, basis, picks, status = run_lrf(dev, xyz)
    assert status.tolist() == [1, 1, 1] and picks.tolist() == [[0, -1], [100, -1], [0, -1]]
    assert (basis == 0).all()
