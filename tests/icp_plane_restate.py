"""numpy restatement of the point-to-plane ICP contract (the
kernel is csrc/icp_plane.hip, its scalar math include/pcr_icp_plane.h).  The
decisions are icp_restate.evaluate, the fp32 evaluation both contracts share;
the step is the normal equations in numpy's order of summation solved by
np.linalg.solve (LU; the kernel's is the Cholesky of pcr_fgr.h), and
np.linalg.cholesky only decides status 3."""
import numpy as np

import icp_restate as ir

F32 = np.float32
MIN_CORR = 6


def delta(x):
    """pcr_fgr_delta: Rz Ry Rx of the angles x[:3] and the translation x[3:]"""
    sa, ca, sb, cb, sc, cc = (np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]),
                              np.sin(x[2]), np.cos(x[2]))
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx, np.asarray(x[3:], np.float64)


def system(r, t, a, b, nrm, corr):
    """A = sum J J^T and g = sum J r over the correspondences, from the fp32
    moved points Evaluate searched with"""
    ok = corr >= 0
    m = ir.apply32(ir.round12(r, t), a)[ok].astype(np.float64)
    bb = b[corr[ok]].astype(np.float64)
    nn = nrm[corr[ok]].astype(np.float64)
    res = ((m - bb) * nn).sum(axis=1)
    jac = np.concatenate((np.cross(m, nn), nn), axis=1)
    return jac.T @ jac, jac.T @ res


def bad_pivots(amat):
    """the kernel's status-3 rule: some Cholesky pivot is not finite and positive"""
    if not np.isfinite(amat).all():
        return True
    try:
        np.linalg.cholesky(amat)
    except np.linalg.LinAlgError:
        return True
    return False


def icp_pair(xyz1, xyz2, normals2, init=None, max_dist=0.2, max_iters=200, rel_fitness=1e-6,
             rel_rmse=1e-6):
    """One pair: xyz1 [3, n1], xyz2 / normals2 [3, n2] fp32, init [4, 4] fp64
    or None.  Returns the outputs plus conv_margin, as icp_restate.icp_pair."""
    a = np.ascontiguousarray(np.asarray(xyz1, F32).T)
    b = np.ascontiguousarray(np.asarray(xyz2, F32).T)
    nrm = np.ascontiguousarray(np.asarray(normals2, F32).T)
    init = np.eye(4) if init is None else np.asarray(init, np.float64)
    r, t = init[:3, :3].copy(), init[:3, 3].copy()
    if len(a) == 0:
        return dict(transform=init.copy(), corr=np.zeros(0, np.int32), num_corr=0, fitness=0.0,
                    rmse=0.0, iterations=0, status=1, conv_margin=float("inf"))
    res = ir.evaluate(r, t, a, b, max_dist) if len(b) else \
        dict(corr=np.full(len(a), -1, np.int32), num_corr=0, e=0.0, fitness=0.0, rmse=0.0)
    it, status, margin = 0, 2, np.inf
    while it < max_iters:
        if res["num_corr"] < MIN_CORR:
            status = 1
            break
        amat, g = system(r, t, a, b, nrm, res["corr"])
        if bad_pivots(amat):
            status = 3
            break
        rd, td = delta(-np.linalg.solve(amat, g))
        r, t = rd @ r, rd @ t + td
        it += 1
        prev, res = res, ir.evaluate(r, t, a, b, max_dist)
        df, dr = abs(prev["fitness"] - res["fitness"]), abs(prev["rmse"] - res["rmse"])
        margin = min(margin, abs(df - rel_fitness), abs(dr - rel_rmse))
        if df < rel_fitness and dr < rel_rmse:
            status = 0
            break
    tr = np.eye(4)
    tr[:3, :3], tr[:3, 3] = r, t
    return dict(transform=tr, corr=res["corr"], num_corr=res["num_corr"], fitness=res["fitness"],
                rmse=res["rmse"], iterations=it, status=status, conv_margin=float(margin))


def icp(xyz1, xyz2, normals2, init=None, **kw):
    """The batch: stacked per-pair results, conv_margin the least over the pairs."""
    res = [icp_pair(xyz1[q], xyz2[q], normals2[q], None if init is None else init[q], **kw)
           for q in range(len(xyz1))]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ir.KEYS}
    for k in ("num_corr", "iterations", "status"):
        out[k] = out[k].astype(np.int32)
    out["conv_margin"] = min(r["conv_margin"] for r in res)
    return out


# ------------------------------------------------------------ synthetic pairs
def ellipsoid(rng, n, axes=(1.0, 0.8, 0.6)):
    """n points on the ellipsoid with semi-axes `axes` (a uniform direction,
    scaled) and their analytic outward unit normals -> [n, 3], [n, 3]"""
    ax = np.asarray(axes, np.float64)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = u * ax
    nrm = pts / (ax * ax)
    return pts, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def make_pair(rng, n1, n2, degrees=5.0, tnorm=0.03, axes=(1.0, 0.8, 0.6)):
    """Source points on the ellipsoid (fp32); the target is a permuted
    superset (n2 >= n1) or subset of them moved by gt, with the moved analytic
    normals.  -> xyz1 [3, n1], xyz2 [3, n2], normals2 [3, n2], gt [4, 4]"""
    pts, nrm = ellipsoid(rng, max(n1, n2), axes)
    a = pts[:n1].astype(F32)
    pts[:n1] = a  # the targets are the rounded sources, moved
    gt = ir.motion(rng, degrees, tnorm)
    sel = rng.permutation(max(n1, n2))[:n2] if n2 < n1 else rng.permutation(n2)
    tgt = pts[sel] @ gt[:3, :3].T + gt[:3, 3]
    tn = nrm[sel] @ gt[:3, :3].T
    return (np.ascontiguousarray(a.T), np.ascontiguousarray(tgt.T.astype(F32)),
            np.ascontiguousarray(tn.T.astype(F32)), gt)


def make_batch(seed, p, n1, n2, **kw):
    rng = np.random.default_rng(seed)
    pairs = [make_pair(rng, n1, n2, **kw) for _ in range(p)]
    return tuple(np.stack([pr[k] for pr in pairs]) for k in range(4))


def sampling_pair(seed, n1=400, n2=4000, degrees=5.0, tnorm=0.03, axes=(1.0, 0.8, 0.6)):
    """Two independent samplings of one ellipsoid: no source point has its
    counterpart in the target.  -> xyz1, xyz2, normals2, gt"""
    rng = np.random.default_rng(seed)
    a, _ = ellipsoid(rng, n1, axes)
    b, nb = ellipsoid(rng, n2, axes)
    gt = ir.motion(rng, degrees, tnorm)
    tgt = b @ gt[:3, :3].T + gt[:3, 3]
    tn = nb @ gt[:3, :3].T
    return (np.ascontiguousarray(a.T.astype(F32)), np.ascontiguousarray(tgt.T.astype(F32)),
            np.ascontiguousarray(tn.T.astype(F32)), gt)


def planar_pair(seed, n1=64, n2=96):
    """A target on the plane z = 0.25 with the normals (0, 0, 1): row 2 of
    every J is an exact zero (m0 * 0 - m1 * 0), so the third pivot is 0."""
    rng = np.random.default_rng(seed)
    b = np.c_[rng.uniform(-1, 1, (n2, 2)), np.full(n2, 0.25)].astype(F32)
    a = b[rng.permutation(n2)[:n1]] + np.array([0.01, -0.02, 0.03], F32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], F32), (n2, 1))
    return (np.ascontiguousarray(a.T.astype(F32)), np.ascontiguousarray(b.T),
            np.ascontiguousarray(nrm.T))


def transform_error(tr, gt):
    return float(np.abs(np.asarray(tr)[:3] - np.asarray(gt)[:3]).max())
