"""numpy / fp64 restatement of the TEASER-style robust registration contract
(the kernels are csrc/teaser.hip, their scalar math
include/pcr_teaser.h and the edge length and rotation solve of
include/pcr_rigid.h).  The edge test, the weight update and the endpoints are
restated operation for operation (decisions hang on them).  The rest is
deliberately another computation where the contract allows one: the clique
search works on Python integers as bit sets; the weights are kept as an array
(the kernel recomputes them from the previous rotation); the rotation is
the SVD solution of Wahba's problem (the kernel's is Horn's quaternion method);
the vote sorts the endpoints and evaluates every midpoint at once as a matrix;
all sums are numpy's, ascending or descending (`order`).  It also carries an
exact maximum clique by Bron-Kerbosch with pivoting, for small graphs."""
import numpy as np

from icp_restate import ball, motion
from rigid_restate import rre_rte  # noqa: F401 (for the tests)

F32 = np.float32
DEFAULTS = dict(noise_bound=0.02, cbar2=1.0, gnc_factor=1.4, max_iters=100, cost_threshold=1e-12,
                seeds=0, inlier_selection=True)
KEYS = ("transform", "clique", "clique_size", "inliers", "num_inliers", "iterations", "status")


def bounds(noise_bound, cbar2):
    """beta, rho"""
    b = np.float64(noise_bound) * np.sqrt(np.float64(cbar2))
    return 2.0 * b, b


def lengths(x):
    """[m, m] fp64 pcr_rigid_dist between the rows of the fp32 points x [m, 3]"""
    d = x.astype(np.float64)
    d = d[None, :, :] - d[:, None, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def graph(a32, b32, beta):
    """the adjacency matrix [m, m] bool"""
    with np.errstate(all="ignore"):
        adj = np.abs(lengths(a32) - lengths(b32)) <= beta  # a NaN compares false
    np.fill_diagonal(adj, False)
    return adj


def bit_rows(adj):
    """row i as a Python integer, bit j = adj[i, j]"""
    return [int.from_bytes(np.packbits(r, bitorder="little").tobytes(), "little") for r in adj]


def members(bits):
    out = []
    while bits:
        low = bits & -bits
        out.append(low.bit_length() - 1)
        bits ^= low
    return out


def greedy_clique(adj, seeds=0):
    """the contract's bounded search -> ascending slots"""
    m = len(adj)
    if m == 0:
        return []
    deg = adj.sum(axis=1)
    order = np.array(sorted(range(m), key=lambda i: (-int(deg[i]), i)))
    rows = bit_rows(adj[np.ix_(order, order)])  # in rank order: the best rank is the lowest bit
    best = []
    for r in range(m if seeds == 0 else min(seeds, m)):
        c, p = [r], rows[r]
        while p:
            u = (p & -p).bit_length() - 1
            c.append(u)
            p &= rows[u]
        if len(c) > len(best):  # strict: the best-ranked seed on ties
            best = c
    return sorted(int(order[u]) for u in best)


def max_clique_size(adj):
    """exact, for small graphs: Bron-Kerbosch with pivoting on integer sets"""
    rows = bit_rows(adj)
    best = 0

    def expand(size, p, x):
        nonlocal best
        if not p and not x:
            best = max(best, size)
            return
        if size + bin(p).count("1") <= best:
            return
        pivot = max(members(p | x), key=lambda u: bin(p & rows[u]).count("1"))
        for v in members(p & ~rows[pivot]):
            expand(size + 1, p & rows[v], x & rows[v])
            p &= ~(1 << v)
            x |= 1 << v

    expand(0, (1 << len(rows)) - 1, 0)
    return best


def weights(r2, mu, nu2):
    """pcr_teaser_weight, elementwise"""
    hi = ((mu + 1.0) / mu) * nu2
    lo = (mu / (mu + 1.0)) * nu2
    with np.errstate(all="ignore"):
        mid = np.sqrt(((nu2 * mu) * (mu + 1.0)) / r2) - mu
    return np.where(r2 >= hi, 0.0, np.where(r2 <= lo, 1.0, mid))


def wahba(h):
    """R maximising sum w v . (R u) for h = sum w u v^T; det R = +1"""
    u, _, vt = np.linalg.svd(h)
    d = 1.0 if np.linalg.det(vt.T @ u.T) >= 0 else -1.0
    return vt.T @ np.diag([1.0, 1.0, d]) @ u.T


def rotation(a, b, nu2, gnc_factor, max_iters, cost_threshold, order=1):
    """GNC-TLS over the TIMs of the fp64 points a, b [k, 3] -> R, iterations,
    status (0, 2 or 3)"""
    i, j = np.triu_indices(len(a), 1)
    u, v = (a[j] - a[i])[::order], (b[j] - b[i])[::order]
    w = np.ones(len(u))
    prev, mu = np.inf, 0.0
    for it in range(1, max_iters + 1):
        h = np.einsum("t,ti,tj->ij", w, u, v)
        if not np.isfinite(h).all():  # non-finite points: so is max r^2
            return np.eye(3), it, 2
        r = wahba(h)
        e = v - u @ r.T
        r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        if it == 1:
            mx = r2.max()  # a NaN stays
            if not np.isfinite(mx):
                return np.eye(3), it, 2
            with np.errstate(all="ignore"):
                mu = 1.0 / ((2.0 * mx) / nu2 - 1.0)
            if not (mu > 0 and np.isfinite(mu)):
                return r, it, 0
        cost = float((w * r2).sum())
        w = weights(r2, mu, nu2)
        mu = mu * gnc_factor
        diff, prev = abs(cost - prev), cost
        if diff < cost_threshold:
            return r, it, 0
    return r, max_iters, 3


def vote(x, rho, order=1):
    """one axis -> the estimate"""
    k = len(x)
    ends = np.stack((x - rho, x + rho), axis=1).reshape(-1)
    srt = np.lexsort((np.arange(2 * k), ends))  # by value, then by number
    mid = 0.5 * (ends[srt][:-1] + ends[srt][1:])
    xo = x[::order]
    inside = np.abs(xo[None, :] - mid[:, None]) <= rho
    n = inside.sum(axis=1)
    with np.errstate(all="ignore"):
        est = np.where(n > 0, (inside * xo[None, :]).sum(axis=1) / n, mid)
    d = xo[None, :] - est[:, None]
    cost = np.where(n > 0, np.minimum(d * d, rho * rho).sum(axis=1), np.inf)
    return float(est[int(np.argmin(cost))])  # the first of the minima


def teaser_pair(xyz1, xyz2, idx1, idx2, m, order=1, **kw):
    """One pair.  xyz1 [3, n1], xyz2 [3, n2] fp32; idx rows [n1]; m = count.
    order: +1 / -1, the direction of every sum."""
    kw = dict(DEFAULTS, **kw)
    xyz1, xyz2 = np.asarray(xyz1, F32), np.asarray(xyz2, F32)
    n1, n2 = xyz1.shape[1], xyz2.shape[1]
    m = min(max(int(m), 0), n1)
    i1 = np.clip(np.asarray(idx1[:m], np.int64), 0, n1 - 1)
    i2 = np.clip(np.asarray(idx2[:m], np.int64), 0, n2 - 1)
    a32 = np.ascontiguousarray(xyz1[:, i1].T)
    b32 = np.ascontiguousarray(xyz2[:, i2].T)
    beta, rho = bounds(kw["noise_bound"], kw["cbar2"])
    if kw["inlier_selection"]:
        cl = greedy_clique(graph(a32, b32, beta), kw["seeds"])
    else:
        cl = list(range(m))
    k = len(cl)
    clique = np.full(n1, -1, np.int32)
    clique[:k] = cl
    out = dict(transform=np.eye(4), clique=clique, clique_size=k, inliers=np.zeros(n1, np.int32),
               num_inliers=0, iterations=0, status=0)
    if k < 3:
        out["status"] = 1
        return out
    a, b = a32[cl].astype(np.float64), b32[cl].astype(np.float64)
    with np.errstate(all="ignore"):
        r, out["iterations"], out["status"] = rotation(
            a, b, beta * beta, kw["gnc_factor"], kw["max_iters"], kw["cost_threshold"], order)
    if out["status"] == 2:
        return out
    x = b - a @ r.T
    t = np.array([vote(x[:, d], rho, order) for d in range(3)])
    inside = (np.abs(x - t) <= rho).all(axis=1)
    out["transform"][:3, :3] = r
    out["transform"][:3, 3] = t
    out["inliers"][np.asarray(cl)[inside]] = 1
    out["num_inliers"] = int(inside.sum())
    return out


def teaser(xyz1, xyz2, idx1, idx2, count, order=1, **kw):
    """The batch: stacked per-pair results."""
    res = [teaser_pair(xyz1[q], xyz2[q], idx1[q], idx2[q], int(count[q]), order, **kw)
           for q in range(len(count))]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in KEYS}
    for k in KEYS[1:]:
        out[k] = out[k].astype(np.int32)
    return out


def order_gap(xyz1, xyz2, idx1, idx2, count, **kw):
    """The restatement with its sums ascending and descending: (the ascending
    result, the largest difference of the two transforms).  The tests'
    condition for the 1e-8 bound and the exact outputs: a gap <= 1e-11 and
    every other output equal."""
    up = teaser(xyz1, xyz2, idx1, idx2, count, 1, **kw)
    down = teaser(xyz1, xyz2, idx1, idx2, count, -1, **kw)
    for k in KEYS[1:]:
        assert np.array_equal(up[k], down[k]), k
    return up, float(np.abs(up["transform"] - down["transform"]).max())


# ------------------------------------------------------------ synthetic pairs
def make_pair(rng, n1, n2, wrong=0.0, m=None, degrees=40.0, tnorm=0.5, noise=0.0):
    """Source points in the unit ball (rounded to fp32); the target is a
    permuted superset (n2 >= n1) moved by R a + t, each point then moved by up
    to `noise` (uniform in a ball), and rounded to fp32.  Slot s < m pairs
    source s with its counterpart, a fraction `wrong` of the slots with a
    random other target instead.  -> xyz1 [3, n1], xyz2 [3, n2], idx1, idx2
    [n1] (-1 past m), m, gt [4, 4], planted (the slots left correct)"""
    a = ball(rng, n1).astype(F32)
    gt = motion(rng, degrees, tnorm)
    pts = np.concatenate((a.astype(np.float64), ball(rng, n2 - n1)))
    perm = rng.permutation(n2)
    tgt = (pts @ gt[:3, :3].T + gt[:3, 3] + noise * ball(rng, n2))[perm]
    pos = np.empty(n2, np.int64)
    pos[perm] = np.arange(n2)
    m = n1 if m is None else m
    idx1, idx2 = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    idx1[:m] = np.arange(m)
    idx2[:m] = pos[:m]
    bad = rng.permutation(m)[:int(wrong * m)]
    idx2[bad] = (idx2[bad] + rng.integers(1, n2, len(bad))) % n2
    planted = np.setdiff1d(np.arange(m), bad)
    return (np.ascontiguousarray(a.T), np.ascontiguousarray(tgt.T.astype(F32)), idx1, idx2, m, gt,
            planted)


def make_batch(seed, p, n1, n2, **kw):
    """-> xyz1 [p, 3, n1], xyz2 [p, 3, n2], idx1, idx2 [p, n1], count [p] int32,
    gt [p, 4, 4], planted (a list of arrays)"""
    rng = np.random.default_rng(seed)
    pairs = [make_pair(rng, n1, n2, **kw) for _ in range(p)]
    out = [np.stack([pr[k] for pr in pairs]) for k in range(6)]
    out[4] = out[4].astype(np.int32)
    return tuple(out) + ([pr[6] for pr in pairs],)
