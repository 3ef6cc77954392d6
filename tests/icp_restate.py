"""numpy restatement of the point-to-point ICP contract (the
kernel is csrc/icp.hip, its scalar math include/pcr_rigid.h and pcr_sumsq3f).
The decisions -- the moved source point, the squared distance, the nearest
target, the distance test -- are fp32, operation for operation, with fmaf
emulated in long double (as oracle/np_restate.py does); the solve is another
algorithm, the SVD Kabsch of tests/rigid_restate.py (the kernel's is Horn's
quaternion method), and the sums are numpy's, in another order."""
import numpy as np

from rigid_restate import kabsch

F32 = np.float32
LD = np.longdouble


def fmaf(a, b, c):
    """float32 fused multiply-add emulated in 80-bit long double."""
    return (LD(1) * np.asarray(a, F32).astype(LD) * np.asarray(b, F32).astype(LD)
            + np.asarray(c, F32).astype(LD)).astype(F32)


def sumsq3(x, y, z):
    return fmaf(z, z, fmaf(x, x, (np.asarray(y, F32) * np.asarray(y, F32)).astype(F32)))


def round12(r, t):
    """pcr_rigid_round: R row-major, then t, as fp32"""
    return np.r_[np.asarray(r, np.float64).reshape(9), np.asarray(t, np.float64)].astype(F32)


def apply32(t12, a):
    """pcr_rigid_apply on a [n, 3] fp32 -> [n, 3] fp32"""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    return np.stack([fmaf(t12[3 * r], ax, fmaf(t12[3 * r + 1], ay, fmaf(t12[3 * r + 2], az,
                                                                        t12[9 + r])))
                     for r in range(3)], axis=1)


def evaluate(r, t, a, b, max_dist, rows=256):
    """Evaluate(T) of the contract.  a [n1, 3], b [n2, 3] fp32 -> corr [n1]
    int32 (-1: none), M, E (fp64 sum of the fp32 squared distances), fitness,
    rmse."""
    n1 = len(a)
    m = apply32(round12(r, t), a)
    tau2 = F32(max_dist) * F32(max_dist)
    corr = np.full(n1, -1, np.int32)
    dmin = np.full(n1, np.inf, F32)
    for s in range(0, n1, rows):
        mm = m[s:s + rows]
        d2 = sumsq3(mm[:, None, 0] - b[None, :, 0], mm[:, None, 1] - b[None, :, 1],
                    mm[:, None, 2] - b[None, :, 2])
        d2 = np.where(np.isfinite(d2), d2, F32(np.inf))
        j = np.argmin(d2, axis=1)  # the first of the minima: the lowest index
        dj = d2[np.arange(len(mm)), j]
        ok = np.isfinite(dj) & (dj <= tau2)
        corr[s:s + rows] = np.where(ok, j, -1)
        dmin[s:s + rows] = dj
    ok = corr >= 0
    mcount = int(ok.sum())
    e = float(dmin[ok].astype(np.float64).sum())
    return dict(corr=corr, num_corr=mcount, e=e, fitness=mcount / n1,
                rmse=float(np.sqrt(e / mcount)) if mcount else 0.0)


def icp_pair(xyz1, xyz2, init=None, max_dist=0.2, max_iters=200, rel_fitness=1e-6,
             rel_rmse=1e-6):
    """One pair: xyz1 [3, n1], xyz2 [3, n2] fp32, init [4, 4] fp64 or None.
    Returns the outputs plus conv_margin: the least | |d rmse| - rel_rmse | and
    | |d fitness| - rel_fitness | over the convergence tests made."""
    a = np.ascontiguousarray(np.asarray(xyz1, F32).T)
    b = np.ascontiguousarray(np.asarray(xyz2, F32).T)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    init = np.eye(4) if init is None else np.asarray(init, np.float64)
    r, t = init[:3, :3].copy(), init[:3, 3].copy()
    res = evaluate(r, t, a, b, max_dist)
    it, status, margin = 0, 2, np.inf
    while it < max_iters:
        if res["num_corr"] < 3:
            status = 1
            break
        ok = res["corr"] >= 0
        r, t = kabsch(a64[ok], b64[res["corr"][ok]])
        it += 1
        prev, res = res, evaluate(r, t, a, b, max_dist)
        df, dr = abs(prev["fitness"] - res["fitness"]), abs(prev["rmse"] - res["rmse"])
        margin = min(margin, abs(df - rel_fitness), abs(dr - rel_rmse))
        if df < rel_fitness and dr < rel_rmse:
            status = 0
            break
    tr = np.eye(4)
    tr[:3, :3], tr[:3, 3] = r, t
    return dict(transform=tr, corr=res["corr"], num_corr=res["num_corr"], fitness=res["fitness"],
                rmse=res["rmse"], iterations=it, status=status, conv_margin=float(margin))


KEYS = ("transform", "corr", "num_corr", "fitness", "rmse", "iterations", "status")


def icp(xyz1, xyz2, init=None, **kw):
    """The batch: stacked per-pair results, conv_margin the least over the pairs."""
    res = [icp_pair(xyz1[q], xyz2[q], None if init is None else init[q], **kw)
           for q in range(len(xyz1))]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in KEYS}
    out["num_corr"] = out["num_corr"].astype(np.int32)
    out["iterations"] = out["iterations"].astype(np.int32)
    out["status"] = out["status"].astype(np.int32)
    out["conv_margin"] = min(r["conv_margin"] for r in res)
    return out


# ------------------------------------------------------------ synthetic pairs
def ball(rng, n):
    """n points uniform in the unit ball, [n, 3]"""
    a = rng.standard_normal((n, 3))
    return a * (rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(a, axis=1, keepdims=True)


def rotation(rng, degrees):
    """rotation by `degrees` about a random axis (Rodrigues)"""
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    th = np.radians(degrees)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def motion(rng, degrees, tnorm):
    gt = np.eye(4)
    gt[:3, :3] = rotation(rng, degrees)
    d = rng.standard_normal(3)
    gt[:3, 3] = d / np.linalg.norm(d) * tnorm
    return gt


def make_pair(rng, n1, n2, degrees=5.0, tnorm=0.03, noise=0.0, dup=False):
    """Source points in the unit ball (rounded to fp32); the target is a
    permuted superset (n2 >= n1: every source plus n2 - n1 further ball
    points) or subset (n2 < n1) of them, moved by R a + t, plus gaussian
    noise, rounded to fp32.  dup: n2 / 2 distinct targets, the second half of
    the cloud repeating the first.  -> xyz1 [3, n1], xyz2 [3, n2], gt [4, 4]"""
    a = ball(rng, n1).astype(F32)
    gt = motion(rng, degrees, tnorm)
    k = n2 // 2 if dup else n2
    pts = a.astype(np.float64)
    pts = np.concatenate((pts, ball(rng, k - n1))) if k > n1 else pts[rng.permutation(n1)[:k]]
    pts = pts[rng.permutation(k)]
    tgt = pts @ gt[:3, :3].T + gt[:3, 3] + rng.normal(0, 1, (k, 3)) * noise
    if dup:
        tgt = np.concatenate((tgt, tgt))
    return (np.ascontiguousarray(a.T), np.ascontiguousarray(tgt.T.astype(F32)), gt)


def make_batch(seed, p, n1, n2, **kw):
    rng = np.random.default_rng(seed)
    pairs = [make_pair(rng, n1, n2, **kw) for _ in range(p)]
    return tuple(np.stack([pr[k] for pr in pairs]) for k in range(3))
