"""Float64 restatements of the PointNet++ ops (sampling.cu,
neighbor_interpolate.cu) and of the change_coords frame
(pvcnn_classify.py:153-184), and the input families of
test_pointnet2_lrf_cpu.py and test_gpu_pointnet2_lrf_edges.py.

The references are plain numpy float64 written from the operations'
definitions; they share no code with include/pcr_math.h, oracle/ or the
kernels.  Where fp32 and float64 may legitimately order two candidates
differently, the reference says so (an `ambiguous` mask, a `margin`) and the
caller skips or refuses the comparison there; on the integer-lattice families
every distance is exact in fp32 and nothing is skipped.
"""
import functools

import numpy as np

TOL = 1e-5          # tests/test_gpu_ops.py TOL: weights and outputs, absolute
AMBIG_GAP = 1e-5    # relative gap between neighbouring distances below which
                    # the order is left open; fp32 rounds |p - c|^2 to ~2e-7
SKIP_CAP = 0.005    # largest share of ambiguous points a test may skip
LRF_MARGIN = 1e-4   # lrf_f64 decides no closer than this to 0.9 and 1e-5
RANK_GAP = 1e-6     # nor between two norms closer than this, relative


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------- three-NN
def three_nn_f64(points, centers, feats=None):
    """points [b, 3, n], centers [b, 3, m], feats [b, c, m] -> dict of
    idx [b, 3, n], dist [b, 3, n], wgt [b, 3, n], out [b, c, n] (if feats),
    ambiguous [b, n].

    The three nearest centres by squared distance, nearest first, ties by the
    lower index (stable argsort).  A centre enters only with a distance below
    the reference's initial 1e40, i.e. any finite one: a NaN or infinite
    distance never enters, and a slot that stays empty (m < 3 included) keeps
    index 0 and the initial distance.  Weights (1 / d_i) / sum(1 / d_j) with d
    clamped to [1e-10, 1e10]; out = sum_i w_i feats[idx_i]; without centres
    out is 0.  `ambiguous` marks the points where two neighbours among the
    four smallest distances differ by less than AMBIG_GAP relative."""
    P, C = np.asarray(points, np.float64), np.asarray(centers, np.float64)
    b, _, n = P.shape
    m = C.shape[2]
    idx = np.zeros((b, 3, n), np.int64)
    dist = np.full((b, 3, n), np.inf)
    amb = np.zeros((b, n), bool)
    with np.errstate(all="ignore"):
        for q in range(b):
            d = ((P[q][:, :, None] - C[q][:, None, :]) ** 2).sum(axis=0)  # [n, m]
            d = np.where(d < np.inf, d, np.inf)
            d = np.concatenate([d, np.full((n, max(0, 4 - m)), np.inf)], axis=1)
            order = np.argsort(d, axis=1, kind="stable")[:, :4]
            ds = np.take_along_axis(d, order, axis=1)
            idx[q] = np.where(ds[:, :3] < np.inf, order[:, :3], 0).T
            dist[q] = ds[:, :3].T
            gap = ds[:, 1:] - ds[:, :-1]
            amb[q] = (np.isfinite(ds[:, 1:]) & (gap < AMBIG_GAP * ds[:, 1:])).any(axis=1)
    inv = 1.0 / np.clip(dist, 1e-10, 1e10)
    wgt = inv / inv.sum(axis=1, keepdims=True)
    res = {"idx": idx, "dist": dist, "wgt": wgt, "ambiguous": amb, "out": None}
    if feats is not None:
        F = np.asarray(feats, np.float64)
        out = np.zeros((b, F.shape[1], n))
        if m > 0:
            for q in range(b):
                for a in range(3):
                    out[q] += F[q][:, idx[q, a]] * wgt[q, a][None, :]
        res["out"] = out
    return res


def check_three_nn(out, inds, wgts, ref, exact=False):
    """A kernel's or the oracle's (out, inds, wgts) against three_nn_f64's
    `ref`.  Indices and outputs are compared off the ambiguous points (on all
    points with `exact`: integer lattices), weights everywhere: tied distances
    give tied weights.  -> (skipped share, max |weight diff|, max |out diff|);
    the share is asserted <= SKIP_CAP."""
    amb = np.zeros_like(ref["ambiguous"]) if exact else ref["ambiguous"]
    skipped = float(amb.mean()) if amb.size else 0.0
    assert skipped <= SKIP_CAP, "ambiguous share %.4f above %.4f" % (skipped, SKIP_CAP)
    keep = ~amb
    bad = (np.asarray(inds) != ref["idx"]) & keep[:, None, :]
    assert not bad.any(), "indices differ at %d places, first %s" % (
        bad.sum(), np.argwhere(bad)[:3].tolist())
    werr = float(np.abs(np.asarray(wgts, np.float64) - ref["wgt"]).max(initial=0.0))
    assert werr <= TOL, "weights off by %.3g" % werr
    oerr = 0.0
    if ref["out"] is not None:
        diff = np.abs(np.asarray(out, np.float64) - ref["out"])
        assert not np.isnan(diff[np.broadcast_to(keep[:, None, :], diff.shape)
                                 & ~np.isnan(ref["out"])]).any(), "NaN output"
        diff = np.where(np.broadcast_to(keep[:, None, :], diff.shape) & ~np.isnan(ref["out"]),
                        diff, 0.0)
        oerr = float(diff.max(initial=0.0))
        assert oerr <= TOL, "interpolated features off by %.3g" % oerr
    return skipped, werr, oerr


# ------------------------------------------------------------------ FPS
def fps_greedy_check(coords, picks, rtol=1e-5):
    """Property of furthest point sampling, replayed in float64 along the
    given picks (so no sequence can diverge after a near-tie): the first pick
    is point 0, and every later pick is a farthest point from the picks before
    it, to `rtol`.  -> the smallest dist[pick] / max(dist) seen."""
    X = np.asarray(coords, np.float64)
    picks = np.asarray(picks)
    worst = 1.0
    for q in range(X.shape[0]):
        assert picks.shape[1] == 0 or picks[q, 0] == 0
        dist = np.full(X.shape[2], np.inf)
        for j in range(1, picks.shape[1]):
            assert 0 <= picks[q, j] < X.shape[2]
            dist = np.minimum(dist, ((X[q] - X[q][:, picks[q, j - 1], None]) ** 2).sum(axis=0))
            top = dist.max()
            assert dist[picks[q, j]] >= (1.0 - rtol) * top, (
                "cloud %d step %d: picked a point at %.9g, the farthest is at %.9g"
                % (q, j, dist[picks[q, j]], top))
            if top > 0:
                worst = min(worst, dist[picks[q, j]] / top)
    return worst


def fps_lattice_exact(coords, m):
    """The reference's picks where every distance is exact (integer
    coordinates): the largest distance, then the lowest k % 512 (its 512
    threads, the tree keeps the left entry), then the lowest k."""
    X = np.asarray(coords, np.float64)
    b, _, n = X.shape
    out = np.zeros((b, m), np.int32)
    k = np.arange(n)
    order = np.lexsort((k, k % 512))  # by k % 512, then k
    for q in range(b):
        dist = np.full(n, np.inf)
        old = 0
        for j in range(1, m):
            dist = np.minimum(dist, ((X[q] - X[q][:, old, None]) ** 2).sum(axis=0))
            cand = order[dist[order] == dist.max()]
            old = int(cand[0])
            out[q, j] = old
    return out


def lattice_cloud(n, duplicate=True):
    """[2, 3, n] integer lattice; the second cloud swaps the x and y axes.
    With `duplicate`, points k and k + 512 coincide.  Without, all points are
    distinct, and a tie between k1 < 512 <= k2 with k2 % 512 < k1 goes to k2:
    only there does the reference's rule differ from the lowest index."""
    g = np.arange(n)
    xyz = np.stack([g % 11, (g // 11) % 10, g // 110]).astype(np.float32)[None]
    if duplicate and n > 512:
        xyz[:, :, 512:] = xyz[:, :, :n - 512]
    return np.ascontiguousarray(np.concatenate([xyz, xyz[:, [1, 0, 2]]], axis=0))


# ------------------------------------------------------------------ LRF
def lrf_f64(coords, exact_ties=False):
    """change_coords (pvcnn_classify.py:153-184) in float64 with a stable
    descending sort of the norms.  -> (new coords [b, 3, n], picks [b, 2],
    status [b], margin [b]).  status 0, or 1 / 2 for the asserts on base_x and
    on lambda (outputs 0, missing pick -1).  margin is how far the comparisons
    that decided the cloud stayed from their thresholds: |lambda| from 0.9
    (absolute) and the norms from 1e-5 (relative), over base_x and every
    candidate walked.  fp32 code may decide differently where the margin is
    under LRF_MARGIN, so callers compare only above it.  The same holds where
    two neighbours in the walked part of the ranking have norms within
    RANK_GAP relative: the margin is then 0, unless `exact_ties` says that
    equal float64 norms are equal in fp32 too (mirror-symmetric integer-like
    clouds whose mean is exactly 0) and the index decides."""
    X = np.asarray(coords, np.float64)
    b, _, n = X.shape
    out = np.zeros((b, 3, n))
    picks = np.full((b, 2), -1, np.int32)
    status = np.zeros(b, np.int32)
    margin = np.full(b, np.inf)
    for i in range(b):
        nc = X[i] - X[i].mean(axis=1, keepdims=True)
        nr = np.sqrt((nc * nc).sum(axis=0))
        rank = np.argsort(-nr, kind="stable")

        def open_rank(pos):  # is the order of rank[pos] and rank[pos + 1] open?
            if pos + 1 >= n:
                return False
            hi, lo = nr[rank[pos]], nr[rank[pos + 1]]
            if exact_ties and hi == lo:
                return False
            return hi - lo < RANK_GAP * hi or not hi > 0

        picks[i, 0] = rank[0]
        n0 = nr[rank[0]]
        margin[i] = 0.0 if open_rank(0) else abs(n0 - 1e-5) / 1e-5
        if not n0 > 1e-5:
            status[i] = 1
            continue
        bx = nc[:, rank[0]] / n0
        by = None
        for pos, j in enumerate(rank[1:], 1):
            margin[i] = min(margin[i], 0.0 if open_rank(pos) else abs(nr[j] - 1e-5) / 1e-5)
            if nr[j] < 1e-5:
                continue
            cand = nc[:, j] / nr[j]
            lam = float(bx @ cand)
            margin[i] = min(margin[i], abs(abs(lam) - 0.9))
            if -0.9 < lam < 0.9:
                by = cand
                picks[i, 1] = j
                break
        if by is None:
            status[i] = 2
            continue
        bx = bx - by * float(bx @ by)
        bx /= np.linalg.norm(bx)
        bz = np.cross(bx, by)
        bz /= np.linalg.norm(bz)
        out[i] = np.stack([bx, by, bz]) @ nc
    return out, picks, status, margin


F32 = np.float32
LAM = F32(0.9)
EPS = F32(1e-5)


def f32_lambda(px, py, pz=F32(0)):
    """fp32 lambda of candidate (px, py, pz) against base_x = (1, 0, 0):
    px / sqrt(px^2 + py^2 + pz^2), every operation rounded once (the products
    with the zero components of base_x add exact zeros)."""
    px, py, pz = F32(px), F32(py), F32(pz)
    return px / np.sqrt(px * px + py * py + pz * pz)


@functools.lru_cache(maxsize=None)
def _candidate_with_lambda(step):
    """fp32 (px, py) near 1.5 (0.9, sqrt(0.19)) whose f32_lambda is exactly
    0.9f moved `step` floats (-1, 0, +1)."""
    want = LAM
    for _ in range(abs(step)):
        want = np.nextafter(want, F32(2 * step))
    px = F32(1.35) + np.arange(-64, 65).astype(np.float32) * np.spacing(F32(1.35))
    py = F32(0.6538348) + np.arange(-512, 513).astype(np.float32) * np.spacing(F32(0.6538348))
    PX, PY = np.meshgrid(px, py, indexing="ij")
    lam = PX / np.sqrt(PX * PX + PY * PY + F32(0) * F32(0))
    hit = np.argwhere(lam == want)
    assert len(hit), "no fp32 candidate with lambda %r" % want
    i, j = hit[len(hit) // 2]
    return F32(PX[i, j]), F32(PY[i, j]), want


def _symmetric(points):
    """[1, 3, 2k]: each point followed by its mirror image, so the mean is
    exactly 0 and base_x = points[0] / |points[0]|."""
    rows = []
    for p in points:
        rows += [p, [-v for v in p]]
    return np.ascontiguousarray(np.array(rows, np.float32).T[None])


def lrf_lambda_cloud(step, negative=False, clear=0.0):
    """Six points: +-(2, 0, 0) (base_x and its mirror, lambda -1), +-C of norm
    ~1.5 and +-(0, 1, 0) (lambda 0).  C's fp32 lambda is exactly 0.9f moved
    `step` floats, or with `clear` 0.9 + clear in float64.  `negative` lists
    -C before C, so the first candidate sits at the -0.9 edge.  -> (xyz,
    lambda of the first candidate, expected picks)."""
    if clear:
        lam = 0.9 + clear
        px, py = F32(1.5 * lam), F32(1.5 * np.sqrt(1.0 - lam * lam))
        inside = clear < 0
        lam = f32_lambda(px, py)
    else:
        px, py, lam = _candidate_with_lambda(step)
        inside = step < 0
    s = -1.0 if negative else 1.0
    xyz = _symmetric([[2, 0, 0], [s * px, s * py, 0], [0, 1, 0]])
    return xyz, F32(s) * lam, (0, 2 if inside else 4)


def lrf_norm_cloud(v, base_x=False):
    """Norm edges.  base_y: +-(1, 0, 0), +-(0.5, 0, 0) (lambda +-1, refused)
    and +-(0, v, 0): v >= 1e-5f is picked (4), below it nothing qualifies
    (status 2).  base_x: +-(v, 0, 0) and +-(0, v, 0): v <= 1e-5f fails the
    first assert (status 1), above it (0, v, 0) ties base_x's norm, ranks
    after it by index and is picked (2).  -> (xyz, status, picks)."""
    v = F32(v)
    if base_x:
        xyz = _symmetric([[v, 0, 0], [0, v, 0]])
        return (xyz, 0, (0, 2)) if v > EPS else (xyz, 1, (0, -1))
    xyz = _symmetric([[1, 0, 0], [0.5, 0, 0], [0, v, 0]])
    return (xyz, 0, (0, 4)) if not v < EPS else (xyz, 2, (0, -1))


# ------------------------------------------------------- input families
TIE_M = 1030  # one full 1024-centre tile, then a float4 group and a tail of 2
_REGION = 40.0


@functools.lru_cache(maxsize=None)
def nn_tie_centres():
    """-> (points [1, 3, n], centres [1, 3, 1030], expected {query: idx
    triple}).  Integer coordinates throughout, so every fp32 distance is
    exact and the stable float64 argsort is the required answer.

    The background centres lie on a lattice 1000 away.  Each planted group
    has its own region 40 apart on the x axis; r is the region's origin:
      0  centres 8, 9 (one float4 group) at r -+ x, 500 at r + 2y
      1  centres 16, 20 (neighbouring groups) likewise, 501
      2  centres 2, 1026 (across the tile boundary, float4 body), 502
      3  centres 5, 1029 (across the boundary, scalar tail), 503
      4  centre 40 at distance 1, 41 at 2, then 30, 33, 700 and 1027 all at 4
    Queries: every region's origin (the tie at the two best, or four ways at
    the third), origin + y (the tie at slots 1 and 2), the first tied centre
    itself (d = 0), and 300 random lattice points around the regions."""
    q = np.arange(TIE_M)
    ctr = np.stack([q % 32, 1000 + (q // 32) % 32, q // 1024]).astype(np.float32)
    expected = {}
    pts = []

    def plant(i, r, off):
        ctr[:, i] = (r + off[0], off[1], off[2])

    for g, (i, j, k) in enumerate([(8, 9, 500), (16, 20, 501), (2, 1026, 502), (5, 1029, 503)]):
        r = _REGION * g
        plant(i, r, (1, 0, 0))
        plant(j, r, (-1, 0, 0))
        plant(k, r, (0, 2, 0))
        expected[len(pts)] = (i, j, k)   # 1, 1, 4
        pts.append((r, 0, 0))
        expected[len(pts)] = (k, i, j)   # 1, 2, 2
        pts.append((r, 1, 0))
        expected[len(pts)] = (i, j, k)   # 0, 4, 5
        pts.append((r + 1, 0, 0))
    r = _REGION * 4
    plant(40, r, (1, 0, 0))
    plant(41, r, (0, 1, 1))
    for i, off in zip((30, 33, 700, 1027), ((2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0))):
        plant(i, r, off)
    expected[len(pts)] = (40, 41, 30)
    pts.append((r, 0, 0))
    rng = np.random.default_rng(11)
    rand = np.stack([rng.integers(-3, 4 * int(_REGION) + 4, 300), rng.integers(-3, 4, 300),
                     rng.integers(-3, 4, 300)], axis=1)
    pts = np.concatenate([np.array(pts, np.float32), rand.astype(np.float32)])
    points = np.ascontiguousarray(pts.T[None])
    centres = np.ascontiguousarray(ctr[None])
    _ro(points, centres)
    return points, centres, expected


@functools.lru_cache(maxsize=None)
def nn_far_centres():
    """-> (points [2, 3, 300], centres [2, 3, 5]): centre 2 among the Gaussian
    queries, the other four 1e5 .. 4e5 away on every axis, so their squared
    distances (3e10 and up) meet the 1e10 clamp."""
    rng = np.random.default_rng(12)
    pts = rng.standard_normal((2, 3, 300)).astype(np.float32)
    ctr = np.empty((2, 3, 5), np.float32)
    for i, s in zip((0, 1, 3, 4), (3e5, -1e5, 2e5, -4e5)):
        ctr[:, :, i] = s
    ctr[:, :, 2] = rng.standard_normal((2, 3)).astype(np.float32)
    return _ro(pts, ctr)


def special_clouds(n, i_nan, i_inf, seed=0):
    """[3, 3, n] Gaussian clouds: cloud 0 has a NaN y at point i_nan, cloud 1
    a +Inf z at point i_inf, cloud 2 both."""
    xyz = np.random.default_rng(seed + n).standard_normal((3, 3, n)).astype(np.float32)
    xyz[(0, 2), 1, i_nan] = np.nan
    xyz[(1, 2), 2, i_inf] = np.inf
    return xyz


# (n, m): point and centre counts of the generic three-NN cases; m = 1027,
# 2051 and 1025 end a later tile on a scalar tail, 7 and 5 follow a float4
# body in the first tile
NN_GENERIC = ((700, 1027), (300, 7), (1000, 2051), (513, 1024), (513, 1025))


@functools.lru_cache(maxsize=None)
def nn_generic(n, m, c=5, b=2):
    """-> (points, centres, features): Gaussian."""
    rng = np.random.default_rng(1000 * n + m + c)
    return _ro(rng.standard_normal((b, 3, n)).astype(np.float32),
               rng.standard_normal((b, 3, m)).astype(np.float32),
               rng.standard_normal((b, c, m)).astype(np.float32))


def nn_special_cases():
    """-> [(name, points, centres)]: the special values in the queries
    (n = 300 against 1027 Gaussian centres) and in the centres (m = 1027, the
    NaN in the first tile's float4 body, the Inf in the last tile's tail)."""
    rng = np.random.default_rng(13)
    pts = rng.standard_normal((3, 3, 300)).astype(np.float32)
    ctr = rng.standard_normal((3, 3, 1027)).astype(np.float32)
    return [("points", special_clouds(300, 7, 290), ctr),
            ("centres", pts, special_clouds(1027, 6, 1026))]


def below(v):
    return np.nextafter(F32(v), F32(-np.inf))


def above(v):
    return np.nextafter(F32(v), F32(np.inf))


# name -> (xyz [1, 3, n], status, picks): one float on either side of every
# threshold of the frame; checked bit for bit and against these expectations
LRF_EDGES = {}
for _s, _name in ((-1, "inside"), (0, "on"), (1, "outside")):
    for _neg in (False, True):
        _xyz, _lam, _picks = lrf_lambda_cloud(_s, _neg)
        LRF_EDGES["lambda%s0.9-%s" % ("-" if _neg else "+", _name)] = (_xyz, 0, _picks)
for _v, _name in ((below(EPS), "below"), (EPS, "on"), (above(EPS), "above")):
    LRF_EDGES["base_y-norm-%s" % _name] = lrf_norm_cloud(_v)
    LRF_EDGES["base_x-norm-%s" % _name] = lrf_norm_cloud(_v, base_x=True)

# the same constructions moved clear of the thresholds, for lrf_f64
LRF_CLEAR = {}
for _c in (-1.5e-4, 1.5e-4):
    for _neg in (False, True):
        _xyz, _lam, _picks = lrf_lambda_cloud(0, _neg, clear=_c)
        LRF_CLEAR["lambda%s%.5f" % ("-" if _neg else "+", 0.9 + _c)] = (_xyz, 0, _picks)
for _f in (1.0 - 2e-4, 1.0 + 2e-4):
    LRF_CLEAR["base_y-norm-%.4fe-5" % _f] = lrf_norm_cloud(1e-5 * _f)
    LRF_CLEAR["base_x-norm-%.4fe-5" % _f] = lrf_norm_cloud(1e-5 * _f, base_x=True)

LRF_SIZES = ((2, 2), (2, 3), (2, 63), (2, 65), (2, 1025), (300, 64))
# the share of generic clouds lrf_f64 may leave undecided: a walked candidate
# has lambda uniform in [-1, 1], so it falls within LRF_MARGIN of +-0.9 with
# probability 2e-4, and a cloud walks one or two candidates; ten times that
LRF_UNDECIDED_CAP = 0.005


def lrf_generic(b, n):
    rng = np.random.default_rng(7 * n + b)
    return (rng.standard_normal((b, 3, n)) + 0.5).astype(np.float32)


FPS_LINES = (256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)


def fps_generic(b, n):
    return np.random.default_rng(3 * n + b).standard_normal((b, 3, n)).astype(np.float32)


# n -> (i_nan, i_inf): in the cloud with both, the two points keep the initial
# 1e38 and tie; the NaN point has the lower k % 512 (8 < 100, 88 < 100) but
# the higher k, so it wins only under the reference's rule
FPS_SPECIAL = {600: (520, 100), 9000: (600, 100)}


def fps_special_expected(n, m):
    """Point 0, then for ever the point that keeps the initial 1e38: fminf
    drops the NaN distance, and once that point is the last pick every new
    distance is NaN or +Inf."""
    i_nan, i_inf = FPS_SPECIAL[n]
    exp = np.zeros((3, m), np.int32)
    exp[0, 1:] = i_nan
    exp[1, 1:] = i_inf
    exp[2, 1:] = min((i_nan, i_inf), key=lambda k: (k % 512, k))
    return exp


def features_for(centres, c, seed=5):
    b, _, m = centres.shape
    return np.random.default_rng(seed + c + m).standard_normal((b, c, m)).astype(np.float32)
