"""Numpy restatement of the FPFH contract (include/pcr_fpfh.h),
written from the text of Open3D's ComputeFPFHFeature / ComputePairFeatures and
vectorised over points and slots: np.float32 arithmetic throughout (every
operation rounds to fp32 on its own), the fused multiply-adds of pcr_dot3f /
pcr_sumsq3f emulated in long double (oracle/np_restate.py fmaf), numpy's own
float64 arctan2 rounded once to float32, np.add.at for the histograms, and
the only loops the serial sums whose order the contract fixes (the slots of a
neighbour set, the 11 channels of a group).  Also a numpy KNN and the surfaces
the CPU and GPU tests share."""
import numpy as np

from oracle.np_restate import fmaf

F = np.float32
CH = 33
PI_F = F(np.pi)
TWO_PI_F = F(2.0) * PI_F


# ------------------------------------------------------------- contract
def dot3(a, b):
    """pcr_dot3f on [..., 3] arrays: fma(a2, b2, fma(a0, b0, a1 * b1))"""
    return fmaf(a[..., 2], b[..., 2], fmaf(a[..., 0], b[..., 0], a[..., 1] * b[..., 1]))


def cross(a, b):
    """every product and difference rounded to fp32 on its own"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(pi, ni, pj, nj):
    """[..., 3] float32 arrays (broadcast) -> f0, f1, f2 float32"""
    with np.errstate(all="ignore"):
        dp = (pj - pi).astype(F)
        f3 = np.sqrt(dot3(dp, dp))
        a1 = dot3(ni, dp) / f3
        a2 = dot3(nj, dp) / f3
        swap = np.abs(a1) < np.abs(a2)
        sw = swap[..., None]
        n1 = np.where(sw, nj, ni)
        n2 = np.where(sw, ni, nj)
        dp = np.where(sw, -dp, dp)
        v = cross(dp, n1)
        vn = np.sqrt(dot3(v, v))
        v = v / vn[..., None]
        w = cross(n1, v)
        f0 = np.arctan2(dot3(w, n2).astype(np.float64), dot3(n1, n2).astype(np.float64)).astype(F)
        f1 = dot3(v, n2)
        f2 = np.where(swap, -a2, a1)
        flat = (f3 == 0) | (vn == 0)
    zero = F(0.0)
    return (np.where(flat, zero, f0).astype(F), np.where(flat, zero, f1).astype(F),
            np.where(flat, zero, f2).astype(F))


def bin_of(t):
    """floor clamped to [0, 10]; a NaN gives 0"""
    with np.errstate(all="ignore"):
        q = np.floor(t)
        return np.where(q >= 10, 10, np.where(q > 0, q, 0)).astype(np.int64)


def bins(f0, f1, f2):
    with np.errstate(all="ignore"):
        return (bin_of((F(11.0) * (f0 + PI_F)) / TWO_PI_F),
                11 + bin_of((F(11.0) * (f1 + F(1.0))) * F(0.5)),
                22 + bin_of((F(11.0) * (f2 + F(1.0))) * F(0.5)))


def in_set(idx, dist, n, radius):
    """idx, dist [kk, n] -> the mask of N(i) per (slot, point)"""
    r2 = F(radius) * F(radius)
    i = np.arange(n)[None, :]
    with np.errstate(all="ignore"):
        return (idx >= 0) & (idx < n) & (idx != i) & (dist > 0) & (dist <= r2)


def fpfh_cloud(xyz, normals, nbr_idx, nbr_dist, radius):
    """One cloud: xyz, normals [3, n]; nbr_idx, nbr_dist [k, n] -> fpfh
    [33, n], spfh [33, n], nbr_count [n]"""
    n = xyz.shape[1]
    kk = min(nbr_idx.shape[0], n)
    p, nr = np.ascontiguousarray(xyz.T, F), np.ascontiguousarray(normals.T, F)
    idx = np.asarray(nbr_idx[:kk], np.int64)
    dist = np.asarray(nbr_dist[:kk], F)
    valid = in_set(idx, dist, n, radius)                       # [kk, n]
    j = np.where(valid, idx, 0)
    f0, f1, f2 = pair_features(p[None], nr[None], p[j], nr[j])  # [kk, n]
    counts = np.zeros((n, CH), np.int64)
    who = np.broadcast_to(np.arange(n)[None, :], valid.shape)[valid]
    for ch in bins(f0, f1, f2):
        np.add.at(counts, (who, ch[valid]), 1)
    m = valid.sum(axis=0)
    assert np.array_equal(counts.sum(axis=1), 3 * m)
    with np.errstate(all="ignore"):
        spfh = np.where(m[:, None] > 0, counts.astype(F) * (F(100.0) / m.astype(F))[:, None],
                        F(0.0)).astype(F)
        acc = np.zeros((n, CH), F)
        for s in range(kk):  # ascending slot
            term = spfh[j[s]] / dist[s][:, None]
            acc = np.where(valid[s][:, None], acc + term, acc).astype(F)
        out = np.empty((n, CH), F)
        for g in range(3):
            sl = slice(11 * g, 11 * g + 11)
            tot = np.zeros(n, F)
            for c in range(11 * g, 11 * g + 11):  # ascending channel
                tot = tot + acc[:, c]
            scale = (F(100.0) / tot)[:, None]
            out[:, sl] = np.where((tot != 0)[:, None], acc[:, sl] * scale, acc[:, sl]) + spfh[:, sl]
    return (np.ascontiguousarray(out.T), np.ascontiguousarray(spfh.T), m.astype(np.int32))


def fpfh(xyz, normals, nbr_idx, nbr_dist, radius):
    """[b, 3, n] clouds with [b, k, n] lists -> fpfh [b, 33, n], spfh
    [b, 33, n], nbr_count [b, n]"""
    per = [fpfh_cloud(xyz[q], normals[q], nbr_idx[q], nbr_dist[q], radius)
           for q in range(xyz.shape[0])]
    return tuple(np.stack([r[a] for r in per]) for a in range(3))


def knn(xyz, k):
    """The lists of pcr_knn_forward for clouds against themselves: [b, 3, n] ->
    dist [b, k, n] (squared, ascending, ties by index; 10000 past n), idx
    [b, k, n] (0 past n)"""
    xyz = np.asarray(xyz, F)
    b, _, n = xyz.shape
    dist = np.full((b, k, n), F(10000.0))
    idx = np.zeros((b, k, n), np.int32)
    kk = min(k, n)
    for q in range(b):
        t = (xyz[q][:, :, None] - xyz[q][:, None, :]).astype(F)
        with np.errstate(all="ignore"):
            d = fmaf(t[2], t[2], fmaf(t[1], t[1], t[0] * t[0]))
        key = np.where(d < F(10000.0), d, np.inf)  # a NaN or a far point sorts last
        order = np.argsort(key, axis=1, kind="stable")[:, :kk]
        got = np.take_along_axis(key, order, axis=1)
        keep = np.isfinite(got)
        dist[q, :kk] = np.where(keep, np.take_along_axis(d, order, axis=1), F(10000.0)).T
        idx[q, :kk] = np.where(keep, order, 0).T
    return dist, idx


# --------------------------------------------------------------- inputs
AXES = np.array([1.0, 0.8, 0.6])
BUMPS = (((0.55, 0.35, 0.30), 0.30, 0.25), ((-0.40, 0.50, -0.25), -0.22, 0.30),
         ((0.20, -0.55, 0.35), 0.26, 0.22))


def implicit(x):
    """The surface is implicit(x) = 0: an ellipsoid with three different
    semi-axes plus three offset Gaussian bumps (no symmetry).  x [..., 3]
    float64 -> the value and its gradient"""
    val = ((x / AXES) ** 2).sum(axis=-1) - 1.0
    grad = 2.0 * x / AXES ** 2
    for c, h, s in BUMPS:
        d = x - np.array(c)
        e = h * np.exp(-(d * d).sum(axis=-1) / (2.0 * s * s))
        val = val - e
        grad = grad + e[..., None] * d / (s * s)
    return val, grad


def surface(n, seed, cap=None):
    """n seeded points of the surface and their analytic unit normals, fp32
    [3, n] each: random directions from the origin (within `cap` radians of a
    fixed axis when given), each ray cut with the surface by bisection"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    if cap is not None:
        axis = np.array([0.48, 0.6, 0.64])
        while True:
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            bad = u @ axis < np.cos(cap)
            if not bad.any():
                break
            u[bad] = rng.standard_normal((int(bad.sum()), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lo, hi = np.full(n, 0.05), np.full(n, 4.0)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        inside = implicit(u * mid[:, None])[0] < 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    x = (u * (0.5 * (lo + hi))[:, None]).astype(F)
    g = implicit(x.astype(np.float64))[1]
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.ascontiguousarray(x.T), np.ascontiguousarray(g.T.astype(F))


def motion(seed, degrees=50.0, tnorm=0.4):
    """a seeded rigid motion [4, 4] float64"""
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.radians(degrees)
    kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    t = rng.standard_normal(3)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * kx @ kx
    out[:3, 3] = tnorm * t / np.linalg.norm(t)
    return out


def moved_copy(xyz, normals, seed):
    """The cloud under a seeded rigid motion and a seeded permutation, rounded
    to fp32 -> xyz2, normals2 [3, n], perm (point perm[s] of the cloud is point
    s of the copy), gt [4, 4]"""
    gt = motion(seed)
    perm = np.random.default_rng(seed + 1).permutation(xyz.shape[1])
    x2 = (gt[:3, :3] @ xyz.astype(np.float64) + gt[:3, 3:4])[:, perm]
    n2 = (gt[:3, :3] @ normals.astype(np.float64))[:, perm]
    return (np.ascontiguousarray(x2.astype(F)), np.ascontiguousarray(n2.astype(F)), perm, gt)


# (b, n, k, radius) of the CPU and GPU tests: n on both sides of the 64-point
# tile and several tiles, k on both sides of the 32-slot chunk and at its
# limits, n < k, b = 3; radii that cut the lists for some points and not others
SHAPES = [(1, 1, 1, 0.5), (3, 1, 2, 0.5), (1, 2, 1, 2.0), (3, 2, 33, 2.0), (1, 63, 2, 0.6),
          (3, 63, 64, 0.6), (1, 64, 33, 0.6), (1, 65, 128, 0.8), (3, 65, 64, 0.5),
          (1, 300, 33, 0.45), (3, 300, 128, 0.6), (1, 1100, 64, 0.3), (3, 1100, 2, 0.3),
          (1, 1100, 128, 0.35)]

_cache = {}


def shape_inputs(b, n, k):
    """xyz, normals [b, 3, n] of b different seeded surfaces and their numpy
    KNN lists idx, dist [b, k, n]; computed once per shape"""
    key = (b, n, k)
    if key not in _cache:
        clouds = [surface(n, seed=100 * n + 7 * q + k) for q in range(b)]
        xyz = np.stack([c[0] for c in clouds])
        nrm = np.stack([c[1] for c in clouds])
        dist, idx = knn(xyz, k)
        _cache[key] = (xyz, nrm, idx, dist)
    return _cache[key]


def salted_inputs():
    """b = 2, n = 300, k = 33 lists salted with -1, n, INT_MAX, INT_MIN and
    with NaN, negative, zero and infinite distances; and a duplicated point"""
    xyz, nrm, idx, dist = (a.copy() for a in shape_inputs(2, 300, 33))
    xyz[1, :, 40] = xyz[1, :, 41]
    dist, idx = knn(xyz, 33)
    rng = np.random.default_rng(8)
    flat_i, flat_d = idx.reshape(-1), dist.reshape(-1)
    where = rng.permutation(flat_i.size)
    for a, v in enumerate((-1, 300, 2 ** 31 - 1, -2 ** 31, 301, -300)):
        flat_i[where[a * 150:(a + 1) * 150]] = v
    for a, v in enumerate((np.nan, -1.0, 0.0, np.inf, -0.0)):
        flat_d[where[1000 + a * 150:1000 + (a + 1) * 150]] = v
    return xyz, nrm, idx, dist, 0.45


def listers(idx, dist, n, radius, p):
    """the mask [n] of point p and the points with p in their N(i)"""
    kk = min(idx.shape[0], n)
    hit = (in_set(idx[:kk].astype(np.int64), dist[:kk], n, radius) & (idx[:kk] == p)).any(axis=0)
    hit[p] = True
    return hit


def mutual_nn(f1, f2):
    """Feature-space mutual nearest neighbours of [c, n1] and [c, n2] features
    -> idx1, idx2 (ascending idx1).  The matching's contract in numpy
    (include/pcr_math.h pcr_match_sqnorm / pcr_match_diff): fp32, every sum
    over the channels a chain of fused multiply-adds in ascending channel,
    diff = (sq1 + sq2) - 2 dot, the first index among equal minima.  At FPFH
    magnitudes (sq ~ 1e5) a point and its copy differ by less than the fp32
    rounding of diff, so the order of the operations decides near ties and a
    float64 matcher would not count what the device counts."""
    a, b = np.ascontiguousarray(f1.T, F), np.ascontiguousarray(f2.T, F)

    def sqnorm(x):
        s = np.zeros(x.shape[0], F)
        for c in range(x.shape[1]):
            s = fmaf(x[:, c], x[:, c], s)
        r = np.sqrt(s)
        return r * r
    dot = np.zeros((a.shape[0], b.shape[0]), F)
    for c in range(a.shape[1]):
        dot = fmaf(a[:, c, None], b[None, :, c], dot)
    d = (sqnorm(a)[:, None] + sqnorm(b)[None, :]) - F(2.0) * dot
    assert d.dtype == F and np.isfinite(d).all()
    c12, c21 = d.argmin(axis=1), d.argmin(axis=0)
    i1 = np.nonzero(c21[c12] == np.arange(len(c12)))[0]
    return i1.astype(np.int32), c12[i1].astype(np.int32)


def assert_same_bits(got, exp, what=""):
    g = np.ascontiguousarray(got)
    e = np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, (what, g.shape, e.shape, g.dtype, e.dtype)
    if g.dtype == F:
        g, e = g.view(np.uint32), e.view(np.uint32)
    bad = np.argwhere(g != e)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())
